// The launch plan of every bf16 GEMM: which kernel, how many K-slices, which tiles go where.  Host only — no HIP types, launches nothing, asks
// no device: gemm_plan() is a pure function of the problem's shape and the tuning knobs, the launchers (gemm.hip, gemm256.hip, gemm_ring*.hip)
// execute its result, vila_gemm_plan_describe() prints it, and tests/test_gemm_plan_cpu.py compiles this header alone with g++.
#pragma once
#include <cstddef>
#include <cstdint>

// The chip's width in CUs.  A constant, not a device query: the thresholds below were measured on the 256-CU MI355X and move with it —
//   one 512-thread 256x256 block per CU: K-slices fill 256 block slots; a GEMM is "whole rounds" of 256 tiles plus a tail
//   two 3-stage ring blocks per CU: the short-prompt ring split-K fills 2 x 256 slots
//   GEMM_256_MIN_TILES (150 of 256 tiles make the 256x256 kernel worth its round), GEMM_TAIL_MAX (a tail above ~1/3 of a round is cheaper
//   left alone; the gate/up tail form takes up to half a round), GEMM_RING64_MAX_TILES128 (the 128x64 ring wins while its grid fits about
//   one round of the 512 resident blocks; GEMM_RING64_MAX_TILES, the same bound in 128x64 tiles, is kept as measured but cannot bind:
//   fewer than 270 tiles of 128^2 are at most 538 of 128x64), GEMM_REG64_MAX_TILES (register-staged 128x64 below 320 tiles of 128^2)
constexpr int GEMM_CUS = 256;
constexpr int GEMM_256_MIN_TILES = 150;
constexpr int GEMM_TAIL_MAX = 96;
constexpr int GEMM_RING64_MAX_TILES = 560;
constexpr int GEMM_RING64_MAX_TILES128 = 270;
constexpr int GEMM_REG64_MAX_TILES = 320;

enum { GEMM_EPI_NONE = 0, GEMM_EPI_GELU_TANH = 1, GEMM_EPI_GELU_ERF = 2, GEMM_EPI_GATEUP = 3 };      // = kernels.h EPI_*

enum GemmFamily {
    GF_256 = 0,          // 256x256 LDS-DMA kernel, whole grid
    GF_256_SLICED,       // ... K-sliced over grid.y into fp32 slabs + a reduce
    GF_256_HYBRID,       // ... whole rounds, then the tail tiles K-sliced (plain GEMMs: compact per-tile slabs; gate/up: whole tile columns)
    GF_CM,               // the same three with a contraction-major operand (dgrad / wgrad)
    GF_CM_SLICED,
    GF_CM_HYBRID,
    GF_RING,             // LDS-DMA ring: `ring` = 3 (128x64, 3 stages) / 4 (128x64, 4 stages) / 8 (128x128, 2 stages), `pipe` = 0 plain / 2
    GF_RING_SPLITK,      // K-sliced 128x64 ring for short prompts
    GF_REG_128x128,      // register-staged kernels of gemm.hip
    GF_REG_128x64,
    GF_REG_256x128,
};
enum GemmReduce { GR_NONE = 0, GR_PLAIN, GR_NORM, GR_ROPE, GR_TAIL, GR_GATEUP };

struct GemmPlan {
    int family = GF_REG_128x128;
    int splits = 1, per = 0;             // K-slices (grid.y of the sliced launch) and K-tiles per slice (the last slice takes the remainder)
    int n_full = 0, n_tail = 0;          // tiles (grid.x) of the whole launch; tile count of the sliced tail launch, whose first tile id is n_full
    int col0 = 0, tail_cols = 0;         // gate/up tail form: first output column and width of the tail
    int ex = 0, bm = 256, group = 0;     // 256x256 kernel: extra row fragment, tile height, tile order (gemm256_kernel.h)
    int sched = 0;                       // 256x256 kernel: forced K-loop schedule (0 = each layout's default)
    int ring = 0, pipe = 0;
    int reduce = GR_NONE;
};

// Every tuning value the plan reads.  -1 = "ask the environment" (the library fills those once, gemm.hip gemm_knobs(); a plan made from an
// unfilled value takes the default the environment would give when the variable is unset).
struct GemmKnobs {
    int force_tile = 0;      // vila_gemm_force_tile: 0 auto, 1 = 128x128, 2 = 128x64, 3 = 256x128, 4 = 256x256 LDS-DMA kernel, 5 = split-K, 6 / 7 = 128x64 DMA ring with 4 / 3 stages, 8 = 128x128 DMA ring (2 stages), 11 = K-sliced 128x64 ring (needs a workspace), 12 / 13 / 14 = rings 7 / 8 / 6 with the PIPE 2 fragment schedule whatever VILA_RING_PIPE says, 15 / 16 / 17 = the same three with the plain schedule
    int ring_splitk = -1;    // VILA_RING_SPLITK: 0 = no K-sliced ring for M < 512 (default 1)
    int ring_pipe = -1;      // VILA_RING_PIPE: "0" = the plain fragment schedule, anything else (or unset) = PIPE 2
    int sched = 0;           // vila_gemm_force_sched: 0 = default schedule of each layout; 1 / 2 / 9 = gemm256_kernel.h SCHED, 10 = SCHED 0
    int group = -1;          // vila_gemm_force_group: -1 = gemm256_group's rule, 0 = tm-fastest everywhere, n = groups of n
    int ex = -1;             // vila_gemm_force_ex / VILA_GEMM_EX (default 1): 0 = off, 1 = gemm256_ex_saves_round, 2 = whenever the rows fit (tests)
    int bm = 0;              // vila_gemm_force_bm: 0 = prefer_bm192's rule, 192 / 256 = force that tile height
    int hybrid = 1;          // vila_gemm_force_hybrid: 0 = never cut a GEMM into whole rounds + K-sliced tail
    int fuse_norm = -1;      // vila_gemm_force_fuse_norm / VILA_FUSE_NORM (default 1): 0 = the reduce never takes the next block's normalisation along
};

struct GemmShape {
    int M = 0, N = 0, K = 0;
    int64_t lda = 0, ldw = 0;                    // stored leading dimensions (gemm256_supported, gemm_ring_supported: 32-bit element offsets)
    int epi = GEMM_EPI_NONE, out_f32 = 0, a_cm = 0, b_cm = 0;
    bool ws = false; size_t ws_bytes = 0;        // fp32 workspace given, and its size
    bool norm_offer = false, rope_offer = false; // the caller offers the next block's normalisation / a complete RoPE + KV follow-up (gemm_rope_offer)
};

static inline int gp_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// The slice rule, written once: as many K-slices as `want` (= free block slots / tiles), at most `cap`, each at least `min_per` K-tiles, the
// slabs (`bytes_per_slice` each) inside the workspace; slices need not be equal (the last one takes the remainder: 42 tiles x 6 slices fills
// 252 CUs where 4 would fill 168), so empty trailing slices are dropped.  0 = do not slice.
static inline int k_slices(int kt, int64_t want, int cap, int min_per, size_t bytes_per_slice, size_t ws_bytes) {
    int s = want > cap ? cap : (int)want;
    while (s >= 2 && (gp_cdiv(kt, s) < min_per || (size_t)s * bytes_per_slice > ws_bytes)) --s;
    return s >= 2 ? gp_cdiv(kt, gp_cdiv(kt, s)) : 0;
}

// ---- 256x256 kernel: what its launches must agree on (gemm256_kernel.h has the design notes) ----
static inline bool gemm256_supported(const GemmShape& a) {
    if (a.a_cm && (a.M % 8 != 0 || a.lda % 8 != 0)) return false;
    if (a.b_cm && (a.N % 8 != 0 || a.ldw % 8 != 0)) return false;
    const int64_t ea = a.a_cm ? (int64_t)64 * a.lda + a.M : (int64_t)a.M * a.lda;      // largest 32-bit element offset the DMA lanes form
    const int64_t eb = a.b_cm ? (int64_t)64 * a.ldw + a.N : (int64_t)a.N * a.ldw;
    // a CC operand is read in 16-B chunks along K (K % 8 == 0); a CM operand in whole k-rows (any K)
    if ((!a.a_cm || !a.b_cm) && a.K % 8 != 0) return false;
    return a.K >= 2 * 64 && ea < (1ll << 31) && eb < (1ll << 31);
}
static inline bool gemm_ring_supported(const GemmShape& a) {
    return a.epi != GEMM_EPI_GATEUP && !a.out_f32 && a.K % 8 == 0 && a.K >= 64 && a.N % 4 == 0 && (int64_t)a.M * a.lda < (1ll << 31) &&
           (int64_t)a.N * a.ldw < (1ll << 31);
}
// grouped tile order where a strip would be long (tiles_m > 16); `gateup` = a fused gate/up launch over part of the grid (tail policy): never
static inline int gemm256_group(int tiles_m, int tiles_n, bool gateup, int force = -1) {
    if (gateup || tiles_n < 2) return 0;
    if (force >= 0) return force;
    return tiles_m > 16 ? 4 : 0;
}
// 192-row tiles (BM) when they need fewer tile-times than 256-row tiles: rounds(tiles) x work per tile, a 192-row tile priced at 0.78 of a
// 256-row one (3/4 of the MFMAs on the same B traffic).  force: 0 = this rule, 192 / 256 = that tile height (vila_gemm_force_bm)
static inline bool prefer_bm192(int M, int N, int force) {
    if (force == 192) return true;
    if (force == 256) return false;
    const int t256 = gp_cdiv(M, 256) * gp_cdiv(N, 256), t192 = gp_cdiv(M, 192) * gp_cdiv(N, 256);
    return 0.78 * gp_cdiv(t192, GEMM_CUS) < 0.97 * gp_cdiv(t256, GEMM_CUS);
}
// rows the LAST 256-row tile carries as an extra 16-row fragment (EX kernels): M = 256 k + r, k >= 1, 1 <= r <= 16; else 0.
// ex_mode 0 switches the policy off (A/B measurements: the callers then see cdiv(M, 256) row tiles again)
static inline int gemm256_ex_rows(int M, int ex_mode) {
    const int r = M % 256;
    return (ex_mode != 0 && M > 256 && r >= 1 && r <= 16) ? r : 0;
}
// 256-row tiles of an M-row output under that policy (what every launch policy must count with when it hands tile ranges to EX launches)
static inline int gemm256_tiles_m(int M, int ex_mode) { return gemm256_ex_rows(M, ex_mode) ? M / 256 : gp_cdiv(M, 256); }
// Whole-grid launches take the EX kernel only when dropping the extra row tile saves a ROUND of 256 blocks: its last-row blocks do 12.5 %
// more MFMAs and the kernel carries 16-28 more registers, measured 5-10 % slower than the plain kernel on grids with the same number of
// rounds (M = 3076 x N = 4608: 92 -> 101 us, profiles/r03_gemm_bench_fwd_ex.log); K-sliced launches always take it (fewer tiles = more slices)
static inline bool gemm256_ex_saves_round(int M, int tiles_n, int ex_mode) {
    if (gemm256_ex_rows(M, ex_mode) == 0) return false;
    if (ex_mode == 2) return true;
    return gp_cdiv((M / 256) * tiles_n, GEMM_CUS) < gp_cdiv(gp_cdiv(M, 256) * tiles_n, GEMM_CUS);
}

// the reduce of a K-sliced launch: the q/k/v projection's RoPE + KV scatter, else the next block's normalisation, else bias + residual
static inline int gemm_sliced_reduce(const GemmShape& a, const GemmKnobs& k) {
    if (a.rope_offer) return GR_ROPE;
    if (a.norm_offer && a.N % 8 == 0 && a.N <= 16384 && k.fuse_norm != 0) return GR_NORM;
    return GR_PLAIN;
}

// The 256x256 kernel was chosen (or forced): whole, whole rounds + sliced tail, or the gate/up tail form.
static inline GemmPlan gemm256_plan(const GemmShape& a, const GemmKnobs& k) {
    GemmPlan p;
    const bool cm = a.a_cm || a.b_cm, plain = a.epi == GEMM_EPI_NONE && !a.out_f32;
    const int ex_mode = k.ex < 0 ? 1 : k.ex, kt = gp_cdiv(a.K, 64);
    const int tiles_n = gp_cdiv(a.N, a.epi == GEMM_EPI_GATEUP ? 128 : 256);
    p.family = cm ? GF_CM : GF_256;
    p.sched = (cm || plain) ? k.sched : 0;
    int tiles_m = gp_cdiv(a.M, 256);
    // Tile quantisation: T tiles on 256 CUs cost ceil(T / 256) rounds.  When the last round is short (wgrad of gate/up/down: 1036 tiles =
    // 4 rounds + 12 tiles, i.e. a fifth round for 1 % of the work) the whole rounds run as usual and the tail tiles are sliced over K so that
    // they fill the chip for a fraction of a tile time; their raw sums go to compact per-tile fp32 slabs and meet in a small reduce kernel
    // (bias / residual applied there).
    if (k.sched == 0 && plain && k.hybrid && a.ws && a.N % 4 == 0) {
        const int tiles = tiles_m * tiles_n, full = (tiles / GEMM_CUS) * GEMM_CUS, tail = tiles - full;
        if (full != 0 && tail != 0 && tail <= GEMM_TAIL_MAX && kt >= 16) {
            const int splits = k_slices(kt, GEMM_CUS / tail, 8, 6, (size_t)tail * 65536 * 4, a.ws_bytes);
            if (splits >= 2) {
                p.family = cm ? GF_CM_HYBRID : GF_256_HYBRID;
                p.splits = splits; p.per = gp_cdiv(kt, splits);
                p.n_full = full; p.n_tail = tail;
                p.group = gemm256_group(tiles_m, tiles_n, false, k.group);
                p.reduce = GR_TAIL;
                return p;
            }
        }
    }
    if (!cm && p.sched == 0) {
        if (a.epi == GEMM_EPI_NONE && !a.out_f32 && prefer_bm192(a.M, a.N, k.bm)) { p.bm = 192; tiles_m = gp_cdiv(a.M, 192); }
        else if (gemm256_ex_saves_round(a.M, tiles_n, ex_mode)) { p.ex = 1; tiles_m = a.M / 256; }      // 1..16 leftover rows ride in the last row tile
    }
    p.n_full = tiles_m * tiles_n;
    p.group = gemm256_group(tiles_m, tiles_n, false, k.group);
    // Gate/up with an under-filled LAST round (S = 769: 592 tiles = 2 full rounds of 256 + 80): the full rounds run fused as usual, the
    // tail tiles (whole tile columns) are sliced over K so the last round costs 1/splits of a tile time; raw gate / up sums meet in a small
    // reduce kernel.  At most 4 slices; slabs that do not fit leave the GEMM whole.
    if (a.epi == GEMM_EPI_GATEUP && a.ws) {
        const int full_tn = ((tiles_m * tiles_n) / GEMM_CUS) * GEMM_CUS / tiles_m;                  // tile columns covered by whole rounds
        const int tail_tn = tiles_n - full_tn, tail_tiles = tail_tn * tiles_m;
        if (full_tn > 0 && tail_tiles > 0 && tail_tiles <= GEMM_CUS / 2 && kt >= 16) {
            const int splits = k_slices(kt, GEMM_CUS / tail_tiles, 4, 1, 0, 0);
            const int tc = tail_tn * 128 < a.N - full_tn * 128 ? tail_tn * 128 : a.N - full_tn * 128;      // output columns of the tail
            if (splits >= 2 && (size_t)splits * 2 * a.M * tc * 4 <= a.ws_bytes && tc % 4 == 0) {
                p.family = GF_256_HYBRID;
                p.splits = splits; p.per = gp_cdiv(kt, splits);
                p.n_full = full_tn * tiles_m; p.n_tail = tail_tiles;
                p.col0 = full_tn * 128; p.tail_cols = tc;
                p.group = 0;                                     // partial gate/up launches cut whole tile COLUMNS: never grouped
                p.reduce = GR_GATEUP;
            }
        }
    }
    return p;
}

// K-sliced 256x256 launch over the whole grid: always the EX kernel where the rows fit (fewer tiles = more slices)
static inline GemmPlan gemm256_sliced_plan(const GemmShape& a, const GemmKnobs& k, int splits) {
    GemmPlan p;
    const bool cm = a.a_cm || a.b_cm;
    const int ex_mode = k.ex < 0 ? 1 : k.ex, tiles_n = gp_cdiv(a.N, 256);
    p.family = cm ? GF_CM_SLICED : GF_256_SLICED;
    p.splits = splits; p.per = gp_cdiv(gp_cdiv(a.K, 64), splits);
    p.ex = !cm && gemm256_ex_rows(a.M, ex_mode) != 0;
    const int tiles_m = p.ex ? a.M / 256 : gp_cdiv(a.M, 256);
    p.n_full = tiles_m * tiles_n;
    p.group = gemm256_group(tiles_m, tiles_n, false, k.group);
    p.reduce = gemm_sliced_reduce(a, k);
    return p;
}

static inline GemmPlan gemm_plan(const GemmShape& a, const GemmKnobs& k) {
    const int kt = gp_cdiv(a.K, 64);
    // dgrad / wgrad on the tensors as they lie (contraction-major operands): always the 256x256 kernel, sliced over K when its tiles cannot
    // fill the chip and the caller lent a workspace
    if (a.a_cm || a.b_cm) {
        const int64_t tiles256 = (int64_t)gp_cdiv(a.M, 256) * gp_cdiv(a.N, 256);
        if (a.ws && tiles256 < GEMM_256_MIN_TILES) {
            const int splits = k_slices(kt, GEMM_CUS / tiles256, 8, 8, (size_t)a.M * a.N * 4, a.ws_bytes);
            if (splits >= 2) return gemm256_sliced_plan(a, k, splits);
        }
        return gemm256_plan(a, k);
    }
    int sel = k.force_tile;
    const bool gu = a.epi == GEMM_EPI_GATEUP, plain = a.epi == GEMM_EPI_NONE && !a.out_f32;
    const int ex_mode = k.ex < 0 ? 1 : k.ex;
    const int64_t tiles256 = (int64_t)gemm256_tiles_m(a.M, ex_mode) * gp_cdiv(a.N, gu ? 128 : 256);
    const bool sup256 = gemm256_supported(a), ring_ok = gemm_ring_supported(a);
    if (sel == 4 || (sel == 0 && tiles256 >= GEMM_256_MIN_TILES)) {
        if (sup256) return gemm256_plan(a, k);
        if (sel == 4) sel = 0;
    }
    // under-filled grid of 256^2 tiles (S = 769 prefill: 56 tiles for N = 3584): slice K over grid.y when a workspace is given
    // (M >= 512 for the short contractions; a LONG contraction — down_proj, K = 18944 — is sliced at ANY M: at S = 289 (one image + a 32-token
    // prompt, BASELINE configs[1]'s short prompt) the ring kernel walked 296 K-tiles per block, 149 us per layer, where 2 x 14 tiles x 8 slices
    // take 57 + 11 us incl. the reduce: TTFT 13.2 -> 12.0 ms, profiles/r04_ttft_s289_ab.log; text-only prompts of 64 / 160 rows:
    // profiles/r04_gemm_bench_presmall.log)
    // Measured and rejected (tools/gemm_bench pol, profiles/r02_gemm_bench_policies.log): slicing K four ways for ONE under-filled round with a
    // long contraction (SFT down_proj forward / dgrad of gate and up: 182 tiles, 296 K-tiles -> 728 blocks = 2.84 rounds of a quarter of the
    // work).  The slabs (4 x 44 MB written and read) eat the gain: 488 -> 481, 522 -> 545, 559 -> 544 us.
    if ((sel == 0 || sel == 5) && plain && a.ws && (a.M >= 512 || kt >= 128) && sup256) {
        // as many K-slices as keep every block resident at once (one 512-thread block per CU), at most 8, at least 8 K-tiles each
        int splits = k_slices(kt, GEMM_CUS / tiles256, 8, 8, (size_t)a.M * a.N * 4, a.ws_bytes);
        // K < 8192 (o_proj at S = 769): the DMA ring below does it in one launch at 557 TF/s vs 482 incl. the reduce
        // ... unless the slices are many and still long (ViT fc2 of one image, K = 4304: 20 tiles x 8 slices; with COLD weights — what a
        // forward pass sees — 45.6 -> 33.7 us, tools/gemm_bench precold; the warm numbers above hide that a lone tile's K loop runs at
        // HBM latency)
        // ... or the caller offers the next block's normalisation (o_proj of the prefill -> post-attention RMSNorm): the reduce then replaces
        // the norm launch as well (ring 44.4 + norm 7.7 us against slices + fused reduce, round 6)
        const bool norm_offer = a.norm_offer && a.N % 8 == 0 && a.N <= 16384 && splits >= 4;
        // ... or the q/k/v projection's RoPE + KV scatter (72 tiles -> 54 with the extra row fragment, 4 slices: the reduce replaces rope_kv_kernel)
        const bool rope_offer = a.rope_offer && splits >= 4;
        if (kt < 128 && sel == 0 && !(kt >= 64 && splits >= 6) && !norm_offer && !rope_offer) splits = 0;
        // measured at M = 769 (tools/microbench.py prefill): N=3584,K=18944 233 -> 122 us; N=3584,K=3584 51 -> 41 us;
        // N=4608 (72 tiles) only breaks even, so require at least 4 slices
        if (splits >= 4 || (splits && sel == 5)) return gemm256_sliced_plan(a, k, splits);
    }
    if (sel == 5) sel = 0;
    GemmPlan p;
    // short prompts (M < 512): the K-sliced 128x64 ring fills the 512 resident block slots (two 3-stage blocks per CU), at most 4 slices, at
    // least 8 K-tiles per slice, slabs inside the workspace (measured in round 5, gemm_ring_splitk.hip; VILA_RING_SPLITK=0 turns it off)
    if (plain && a.ws && (sel == 11 || (sel == 0 && k.ring_splitk != 0 && a.M < 512)) && ring_ok) {
        const int64_t tiles = (int64_t)gp_cdiv(a.M, 128) * gp_cdiv(a.N, 64);
        const int splits = k_slices(kt, 2 * GEMM_CUS / tiles, 4, 8, (size_t)a.M * a.N * 4, a.ws_bytes);
        if (splits >= 2) { p.family = GF_RING_SPLITK; p.n_full = (int)tiles; p.splits = splits; p.per = gp_cdiv(kt, splits); p.reduce = GR_PLAIN; return p; }
    }
    // everything below the gemm256 threshold: the LDS-DMA ring kernels (gemm_ring.hip) instead of the one-tile-ahead register staging
    if (!gu && !a.out_f32 && ring_ok) {
        const int64_t tiles_ring = (int64_t)gp_cdiv(a.M, 128) * gp_cdiv(a.N, 64);
        // measured (tools/microbench.py tiles): the 128x64 3-stage ring wins while its grid fits about one round of the 512
        // resident blocks (S=769 q/k/v 473 -> 675 TF/s, o_proj 397 -> 557, ViT fc2 168 -> 297); beyond that the 128x128 2-stage
        // ring takes over from the register-staged 128x128 kernel (SFT ViT shapes 376-590 -> 459-697, 4096^3 810 -> 1015)
        const int64_t tiles128r = (int64_t)gp_cdiv(a.M, 128) * gp_cdiv(a.N, 128);
        int ring = 0;
        if (sel == 12 || sel == 15 || sel == 7 || (sel == 0 && tiles_ring <= GEMM_RING64_MAX_TILES && tiles128r < GEMM_RING64_MAX_TILES128)) ring = 3;
        else if (sel == 14 || sel == 17 || sel == 6) ring = 4;
        else if (sel == 13 || sel == 16 || sel == 8 || sel == 0) ring = 8;
        if (ring) {
            p.family = GF_RING; p.ring = ring; p.n_full = ring == 8 ? (int)tiles128r : (int)tiles_ring;
            p.pipe = (sel >= 12 && sel <= 14) ? 2 : (sel >= 15 && sel <= 17) ? 0 : k.ring_pipe == 0 ? 0 : 2;      // forced tiles 12-17 name the fragment schedule
            return p;
        }
    }
    if (sel >= 6 && sel <= 17) sel = 0;
    if (sel == 0) sel = ((int64_t)gp_cdiv(a.M, 128) * gp_cdiv(a.N, gu ? 64 : 128) < GEMM_REG64_MAX_TILES && !gu) ? 2 : 1;
    if (sel == 2 && gu) sel = 1;
    p.family = sel == 3 ? GF_REG_256x128 : sel == 2 ? GF_REG_128x64 : GF_REG_128x128;
    p.n_full = sel == 3 ? gp_cdiv(a.M, 256) * gp_cdiv(a.N, gu ? 64 : 128) : gp_cdiv(a.M, 128) * gp_cdiv(a.N, sel == 2 ? 64 : gu ? 64 : 128);
    return p;
}

// what launch_gemm's argument checks ask of the shape itself (pointer alignment aside): a plan exists only for these
static inline bool gemm_shape_ok(const GemmShape& a) {
    if (a.M <= 0 || a.N <= 0 || a.K <= 0 || a.N % 4 != 0 || a.lda % 8 != 0 || a.ldw % 8 != 0) return false;
    if (a.a_cm || a.b_cm) return a.epi == GEMM_EPI_NONE && !a.out_f32 && gemm256_supported(a);
    return a.K % 8 == 0 && a.epi >= GEMM_EPI_NONE && a.epi <= GEMM_EPI_GATEUP && !(a.out_f32 && a.epi != GEMM_EPI_NONE);
}

static inline const char* gemm_family_name(int f) {
    static const char* const n[] = {"256", "256_sliced", "256_hybrid", "cm", "cm_sliced", "cm_hybrid", "ring", "ring_splitk", "reg128x128", "reg128x64", "reg256x128"};
    return f >= 0 && f <= GF_REG_256x128 ? n[f] : "?";
}
static inline const char* gemm_reduce_name(int r) {
    static const char* const n[] = {"none", "plain", "norm", "rope", "tail", "gateup"};
    return r >= 0 && r <= GR_GATEUP ? n[r] : "?";
}

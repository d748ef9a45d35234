// C-ABI of libvila_hip.so (include/vila_hip.h): model-level chaining of the kernels on the caller's stream.
#include <stdarg.h>
#include <stdio.h>
#include <vector>
#include "../../include/vila_hip.h"
#include "../../include/vila_hip_tuning.h"
#include "kernels.h"
#include "attn_decode.h"
#include "train.h"
#include "w4.h"

static thread_local char g_err[512] = "";
void vila_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* vila_last_error(void) { return g_err; }
extern "C" int vila_abi_version(void) { return 1; }

namespace {
struct Arena {
    char* base; size_t size, off;
    Arena(void* p, size_t n) : base((char*)p), size(n), off(0) {}
    template <typename T> T* take(size_t count) {
        off = align_up(off, 256);
        T* r = (T*)(base + off);
        off += count * sizeof(T);
        return r;
    }
    bool ok() const { return off <= size; }
};
}  // namespace
hipStream_t vila_stream_enter(void* s);      // (kernels.h) the same for the other translation units
namespace {
// Every entry point takes its device from the stream handle (backward runs on autograd worker threads whose thread-local HIP
// device need not be the caller's): a non-default stream names its device, and the calling thread is switched to it before anything is
// launched.  The lookup is cached per thread and stream, so the steady state costs one compare.
inline hipStream_t S(vila_stream_t s) {
    hipStream_t st = (hipStream_t)s;
    if (st != nullptr) {
        static thread_local hipStream_t last = nullptr;
        static thread_local int last_dev = -1;
        if (st != last) {
            hipDevice_t dev = 0;
            if (hipStreamGetDevice(st, &dev) == hipSuccess) { last = st; last_dev = (int)dev; }
            else (void)hipGetLastError();
        }
        if (st == last && last_dev >= 0) {
            int cur = -1;
            if (hipGetDevice(&cur) == hipSuccess && cur != last_dev) (void)hipSetDevice(last_dev);
        }
    }
    return st;
}
}  // namespace
hipStream_t vila_stream_enter(void* s) { return S((vila_stream_t)s); }
namespace {
inline const bf16_t* B(const void* p) { return (const bf16_t*)p; }
inline bf16_t* B(void* p) { return (bf16_t*)p; }
// q/k/v weights [q_rows | kv_rows | kv_rows, cols] and their biases are views of one fused buffer, in that order
bool qkv_fused(const void* wq, const void* wk, const void* wv, const void* bq, const void* bk, const void* bv, size_t q_rows, size_t kv_rows, size_t cols) {
    return B(wk) == B(wq) + q_rows * cols && B(wv) == B(wk) + kv_rows * cols && B(bk) == B(bq) + q_rows && B(bv) == B(bk) + kv_rows;
}

// the NEXT block's normalisation, offered to a GEMM whose split-K reduce can take it along (kernels.h GemmArgs::norm_*)
struct NextNorm { const void* w = nullptr; const void* b = nullptr; float eps = 0.f; int rms = 0; bf16_t* out = nullptr; int* done = nullptr; };
// the q/k/v projection's follow-up (bias -> RoPE -> K / V into the cache), offered to its GEMM in the same way (kernels.h GemmArgs::rope_*)
struct NextRope { const float* cs = nullptr; const float* sn = nullptr; const int32_t* pos = nullptr; const int32_t* seq = nullptr; bf16_t* kc = nullptr; bf16_t* vc = nullptr;
                  int nq = 0, nkv = 0, hd = 0, max_ctx = 0; int* done = nullptr; };
int gemm(const bf16_t* A, int64_t lda, const void* W, int64_t ldw, const void* bias, const bf16_t* res, int64_t ldr,
         void* C, int64_t ldc, int M, int N, int K, int epi, hipStream_t s, const void* W2 = nullptr, int out_f32 = 0,
         float* ws = nullptr, size_t ws_bytes = 0, int res_mod = 0, const NextNorm* nn = nullptr, const NextRope* nr = nullptr) {
    GemmArgs g;
    if (nr != nullptr) { g.rope_cs = nr->cs; g.rope_sn = nr->sn; g.rope_pos = nr->pos; g.rope_seq = nr->seq; g.rope_kc = nr->kc; g.rope_vc = nr->vc;
                         g.rope_nq = nr->nq; g.rope_nkv = nr->nkv; g.rope_hd = nr->hd; g.rope_max_ctx = nr->max_ctx; g.rope_done = nr->done; }
    if (nn != nullptr) { g.norm_w = B(nn->w); g.norm_b = B(nn->b); g.norm_eps = nn->eps; g.norm_rms = nn->rms; g.norm_out = nn->out; g.norm_done = nn->done; }
    g.ws = ws; g.ws_bytes = ws_bytes; g.res_mod = res_mod;
    g.A = A; g.lda = lda; g.W = B(W); g.ldw = ldw; g.W2 = B(W2); g.bias = B(bias); g.residual = res; g.ldr = ldr;
    g.C = C; g.ldc = ldc; g.out_f32 = out_f32; g.M = M; g.N = N; g.K = K; g.epi = epi;
    return launch_gemm(g, s);
}
}  // namespace

// =================================================================================================
// Vision tower
// =================================================================================================
static inline int vit_kp(const VilaVitShape* s) { return (int)align_up((size_t)s->channels * s->patch * s->patch, 8); }

// fc2 (K = 4304) of one or two images is 20-40 tiles of 256^2: its weights arrive cold from HBM and a tile's K loop runs at memory latency,
// so it is sliced over K (8 slices of one image: 45.6 -> 33.7 us, tools/gemm_bench precold); beyond 2048 rows the tiles fill the chip
static size_t vit_splitk_rows(size_t M) { return M <= 2048 ? M : 0; }
extern "C" size_t vila_vit_workspace_bytes(const VilaVitShape* s, int n_images) {
    const size_t g = s->image / s->patch, M = (size_t)n_images * g * g, D = s->hidden, F = s->inter, Kp = vit_kp(s);
    size_t b = 0;
    b += align_up(M * Kp * 2, 256) + align_up(D * Kp * 2, 256);     // patches, padded conv weight
    b += 2 * align_up(M * D * 2, 256);                               // x, h
    b += align_up(M * 3 * D * 2, 256);                               // qkv
    b += align_up(M * F * 2, 256);                                   // mlp hidden
    b += align_up(vit_splitk_rows(M) * D * 4 * 8, 256);              // fp32 K-slices of fc2 when its 256^2 tiles cannot fill the chip
    return b + 4096;
}

extern "C" int vila_vit_forward(const VilaVitWeights* w, const void* pixels, int n_images, void* out,
                                void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    const VilaVitShape& sh = w->shape;
    hipStream_t s = S(stream);
    VILA_REQUIRE(n_images > 0, "vit: n_images must be positive");
    VILA_REQUIRE(sh.image % sh.patch == 0, "vit: image size %d is not a multiple of patch size %d", sh.image, sh.patch);
    VILA_REQUIRE(sh.hidden % sh.heads == 0, "embed_dim must be divisible by num_heads (got `embed_dim`: %d and `num_heads`: %d).", sh.hidden, sh.heads);
    VILA_REQUIRE(workspace_bytes >= vila_vit_workspace_bytes(&sh, n_images), "vit: workspace too small");
    const int g = sh.image / sh.patch, N = g * g, M = n_images * N, D = sh.hidden, F = sh.inter, hd = D / sh.heads;
    const int Kc = sh.channels * sh.patch * sh.patch, Kp = vit_kp(&sh);
    Arena a(workspace, workspace_bytes);
    bf16_t* patches = a.take<bf16_t>((size_t)M * Kp);
    bf16_t* wpad = a.take<bf16_t>((size_t)D * Kp);
    bf16_t* x = a.take<bf16_t>((size_t)M * D);
    bf16_t* h = a.take<bf16_t>((size_t)M * D);
    bf16_t* qkv = a.take<bf16_t>((size_t)M * 3 * D);
    bf16_t* f = a.take<bf16_t>((size_t)M * F);
    const size_t sk_bytes = vit_splitk_rows(M) * D * 4 * 8;
    float* skws = sk_bytes ? a.take<float>(sk_bytes / 4) : nullptr;
    VILA_REQUIRE(a.ok(), "vit: workspace arena overflow");

    // a2: patch embed = im2col + ONE GEMM over all images (+bias) with the position embedding as a periodic residual operand
    // (row m of the batch reads pos_emb[m % N]): 64 frames are one launch with one tail, not 64
    VILA_TRY(launch_im2col(B(pixels), patches, n_images, sh.channels, sh.image, sh.image, sh.patch, Kp, s));
    VILA_TRY(launch_pad_rows(B(w->patch_w), wpad, D, Kc, Kp, s));
    bf16_t* x0 = (sh.n_layers_run == 0) ? B(out) : x;
    VILA_TRY(gemm(patches, Kp, wpad, Kp, w->patch_b, B(w->pos_emb), D, x0, D, M, D, Kp, EPI_NONE, s, nullptr, 0, nullptr, 0, N));

    int ln1_done = 0;                                           // the previous layer's fc2 reduce already wrote layer_norm1(x) into h
    for (int l = 0; l < sh.n_layers_run; ++l) {
        const VilaVitLayer& L = w->layers[l];
        bf16_t* xo = (l == sh.n_layers_run - 1) ? B(out) : x;   // last layer writes straight into `out`
        if (!ln1_done) VILA_TRY(launch_layernorm(x, B(L.ln1_w), B(L.ln1_b), h, M, D, sh.ln_eps, s));
        ln1_done = 0;
        if (qkv_fused(L.wq, L.wk, L.wv, L.bq, L.bk, L.bv, D, D, D)) {
            VILA_TRY(gemm(h, D, L.wq, D, L.bq, nullptr, 0, qkv, 3 * D, M, 3 * D, D, EPI_NONE, s));
        } else {
            VILA_TRY(gemm(h, D, L.wq, D, L.bq, nullptr, 0, qkv, 3 * D, M, D, D, EPI_NONE, s));
            VILA_TRY(gemm(h, D, L.wk, D, L.bk, nullptr, 0, qkv + D, 3 * D, M, D, D, EPI_NONE, s));
            VILA_TRY(gemm(h, D, L.wv, D, L.bv, nullptr, 0, qkv + 2 * D, 3 * D, M, D, D, EPI_NONE, s));
        }
        AttnArgs at{};
        at.q = qkv; at.k = qkv + D; at.v = qkv + 2 * D; at.o = h;
        at.q_tok_stride = at.k_tok_stride = at.v_tok_stride = 3 * D; at.o_tok_stride = D;
        at.q_head_stride = at.k_head_stride = at.v_head_stride = at.o_head_stride = hd;
        at.cu_seqlens = nullptr; at.n_seq = n_images; at.total_tokens = M; at.max_seqlen = N;
        at.n_q_heads = at.n_kv_heads = sh.heads; at.head_dim = hd; at.causal = 0; at.scale = 1.0f / sqrtf((float)hd);
        at.lse = nullptr;
        VILA_TRY(launch_attn_fwd(at, s));
        VILA_TRY(gemm(h, D, L.wo, D, L.bo, x, D, x, D, M, D, D, EPI_NONE, s));               // x += out_proj(attn)
        VILA_TRY(launch_layernorm(x, B(L.ln2_w), B(L.ln2_b), h, M, D, sh.ln_eps, s));
        VILA_TRY(gemm(h, D, L.fc1_w, D, L.fc1_b, nullptr, 0, f, F, M, F, D, EPI_GELU_TANH, s));
        // x += fc2(gelu(fc1)); where fc2 is K-sliced its reduce takes the NEXT layer's layer_norm1 along (h is free: fc1 has consumed it)
        NextNorm nn;
        if (l + 1 < sh.n_layers_run) { nn.w = w->layers[l + 1].ln1_w; nn.b = w->layers[l + 1].ln1_b; nn.eps = sh.ln_eps; nn.rms = 0; nn.out = h; nn.done = &ln1_done; }
        VILA_TRY(gemm(f, F, L.fc2_w, F, L.fc2_b, x, D, xo, D, M, D, F, EPI_NONE, s, nullptr, 0, skws, sk_bytes, 0, l + 1 < sh.n_layers_run ? &nn : nullptr));
    }
    return 0;
}

// W8A8 vision tower (SURVEY.md §8f row 3 / BASELINE configs[4]): the four linears of every encoder layer run int8 x int8 on the matrix
// cores (per-output-channel weight scales, per-token dynamic activation scales); patch embedding, LayerNorms, attention, biases,
// residual stream stay bf16.  Same call contract as vila_vit_forward.
extern "C" size_t vila_vit_w8a8_workspace_bytes(const VilaVitShape* s, int n_images) {
    const size_t g = s->image / s->patch, M = (size_t)n_images * g * g, F = s->inter, D = s->hidden;
    return vila_vit_workspace_bytes(s, n_images) + align_up(M * (F > D ? F : D), 256) + align_up(M * 4, 256) + 1024;
}
extern "C" int vila_vit_forward_w8a8(const VilaVitWeights* w, const VilaVitLayerW8* ql, const void* pixels, int n_images, void* out,
                                     void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    const VilaVitShape& sh = w->shape;
    hipStream_t s = S(stream);
    VILA_REQUIRE(n_images > 0 && ql != nullptr, "vit_w8a8: n_images must be positive and the int8 layers given");
    VILA_REQUIRE(sh.image % sh.patch == 0 && sh.hidden % sh.heads == 0, "vit_w8a8: bad shape");
    VILA_REQUIRE(sh.hidden % 16 == 0 && sh.inter % 16 == 0, "vit_w8a8: hidden (%d) and intermediate (%d) sizes must be multiples of 16", sh.hidden, sh.inter);
    VILA_REQUIRE(workspace_bytes >= vila_vit_w8a8_workspace_bytes(&sh, n_images), "vit_w8a8: workspace too small");
    const int g = sh.image / sh.patch, N = g * g, M = n_images * N, D = sh.hidden, F = sh.inter, hd = D / sh.heads;
    const int Kc = sh.channels * sh.patch * sh.patch, Kp = vit_kp(&sh);
    Arena a(workspace, workspace_bytes);
    bf16_t* patches = a.take<bf16_t>((size_t)M * Kp);
    bf16_t* wpad = a.take<bf16_t>((size_t)D * Kp);
    bf16_t* x = a.take<bf16_t>((size_t)M * D);
    bf16_t* h = a.take<bf16_t>((size_t)M * D);
    bf16_t* qkv = a.take<bf16_t>((size_t)M * 3 * D);
    bf16_t* f = a.take<bf16_t>((size_t)M * F);
    int8_t* xq = a.take<int8_t>((size_t)M * (F > D ? F : D));
    float* sx = a.take<float>((size_t)M);
    VILA_REQUIRE(a.ok(), "vit_w8a8: workspace arena overflow");
    VILA_TRY(launch_im2col(B(pixels), patches, n_images, sh.channels, sh.image, sh.image, sh.patch, Kp, s));
    VILA_TRY(launch_pad_rows(B(w->patch_w), wpad, D, Kc, Kp, s));
    bf16_t* x0 = (sh.n_layers_run == 0) ? B(out) : x;
    VILA_TRY(gemm(patches, Kp, wpad, Kp, w->patch_b, B(w->pos_emb), D, x0, D, M, D, Kp, EPI_NONE, s, nullptr, 0, nullptr, 0, N));
    for (int l = 0; l < sh.n_layers_run; ++l) {
        const VilaVitLayer& L = w->layers[l];
        const VilaVitLayerW8& Q = ql[l];
        bf16_t* xo = (l == sh.n_layers_run - 1) ? B(out) : x;
        VILA_TRY(launch_layernorm(x, B(L.ln1_w), B(L.ln1_b), h, M, D, sh.ln_eps, s));
        VILA_TRY(launch_quant_rows_i8(h, xq, sx, M, D, s));
        VILA_TRY(launch_gemm_i8(xq, D, (const int8_t*)Q.wqkv_q, D, sx, Q.wqkv_s, B(L.bq), nullptr, 0, qkv, 3 * D, M, 3 * D, D, EPI_NONE, s));
        AttnArgs at{};
        at.q = qkv; at.k = qkv + D; at.v = qkv + 2 * D; at.o = h;
        at.q_tok_stride = at.k_tok_stride = at.v_tok_stride = 3 * D; at.o_tok_stride = D;
        at.q_head_stride = at.k_head_stride = at.v_head_stride = at.o_head_stride = hd;
        at.cu_seqlens = nullptr; at.n_seq = n_images; at.total_tokens = M; at.max_seqlen = N;
        at.n_q_heads = at.n_kv_heads = sh.heads; at.head_dim = hd; at.causal = 0; at.scale = 1.0f / sqrtf((float)hd);
        at.lse = nullptr;
        VILA_TRY(launch_attn_fwd(at, s));
        VILA_TRY(launch_quant_rows_i8(h, xq, sx, M, D, s));
        VILA_TRY(launch_gemm_i8(xq, D, (const int8_t*)Q.wo_q, D, sx, Q.wo_s, B(L.bo), x, D, x, D, M, D, D, EPI_NONE, s));            // x += out_proj(attn)
        VILA_TRY(launch_layernorm(x, B(L.ln2_w), B(L.ln2_b), h, M, D, sh.ln_eps, s));
        VILA_TRY(launch_quant_rows_i8(h, xq, sx, M, D, s));
        VILA_TRY(launch_gemm_i8(xq, D, (const int8_t*)Q.fc1_q, D, sx, Q.fc1_s, B(L.fc1_b), nullptr, 0, f, F, M, F, D, EPI_GELU_TANH, s));
        VILA_TRY(launch_quant_rows_i8(f, xq, sx, M, F, s));
        VILA_TRY(launch_gemm_i8(xq, F, (const int8_t*)Q.fc2_q, F, sx, Q.fc2_s, B(L.fc2_b), x, D, xo, D, M, D, F, EPI_NONE, s));      // x += fc2(gelu(fc1))
    }
    return 0;
}
extern "C" int vila_quant_rows_i8(const void* x, void* q, float* scale, int rows, int cols, vila_stream_t stream) {
    return launch_quant_rows_i8(B(x), (int8_t*)q, scale, rows, cols, S(stream));
}
extern "C" int vila_gemm_w8a8(const void* Aq, int64_t lda, const void* Wq, int64_t ldw, const float* sx, const float* sw, const void* bias,
                              const void* residual, int64_t ldr, void* C, int64_t ldc, int M, int N, int K, int epi, vila_stream_t stream) {
    return launch_gemm_i8((const int8_t*)Aq, lda, (const int8_t*)Wq, ldw, sx, sw, B(bias), B(residual), ldr, B(C), ldc, M, N, K, epi, S(stream));
}

// =================================================================================================
// Projector
// =================================================================================================
extern "C" int vila_proj_out_tokens(int kind, int n_tokens) {
    const int g = (int)(sqrt((double)n_tokens) + 0.5);
    const int k = (kind == VILA_PROJ_MLP_DOWNSAMPLE_3X3_FIX) ? 3 : 2;
    const int gd = (g + k - 1) / k;
    return gd * gd;
}
extern "C" size_t vila_proj_workspace_bytes(const VilaProjWeights* w, int n_images, int n_tokens) {
    const int k = (w->kind == VILA_PROJ_MLP_DOWNSAMPLE_3X3_FIX) ? 3 : 2;
    const size_t T = (size_t)n_images * vila_proj_out_tokens(w->kind, n_tokens);
    const size_t C = w->in_dim, H = w->out_dim;
    return align_up(T * k * k * C * 2, 256) + align_up(T * 3 * C * 2, 256) + 2 * align_up(T * H * 2, 256) + 4096;
}
extern "C" int vila_proj_forward(const VilaProjWeights* w, const void* feat, int n_images, int n_tokens, void* out,
                                 void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    hipStream_t s = S(stream);
    const int g = (int)(sqrt((double)n_tokens) + 0.5);
    VILA_REQUIRE(g * g == n_tokens, "projector: token count %d is not a perfect square", n_tokens);
    VILA_REQUIRE(w->kind >= 0 && w->kind <= 2, "Unknown projector type: %d", w->kind);
    VILA_REQUIRE(workspace_bytes >= vila_proj_workspace_bytes(w, n_images, n_tokens), "projector: workspace too small");
    const int k = (w->kind == VILA_PROJ_MLP_DOWNSAMPLE_3X3_FIX) ? 3 : 2;
    const int T = n_images * vila_proj_out_tokens(w->kind, n_tokens);
    const int C = w->in_dim, H = w->out_dim, C1 = k * k * C;
    Arena a(workspace, workspace_bytes);
    bf16_t* y = a.take<bf16_t>((size_t)T * C1);
    bf16_t* mid = a.take<bf16_t>((size_t)T * 3 * C);
    bf16_t* h1 = a.take<bf16_t>((size_t)T * H);
    VILA_REQUIRE(a.ok(), "projector: workspace arena overflow");
    VILA_TRY(launch_space_to_depth(B(feat), y, n_images, g, C, k, s));
    VILA_TRY(launch_layernorm(y, B(w->ln1_w), B(w->ln1_b), y, T, C1, 1e-5f, s));
    if (k == 2) {
        VILA_TRY(gemm(y, C1, w->fc1_w, C1, w->fc1_b, nullptr, 0, h1, H, T, H, C1, EPI_GELU_ERF, s));
        VILA_TRY(gemm(h1, H, w->fc2_w, H, w->fc2_b, nullptr, 0, out, H, T, H, H, EPI_NONE, s));
    } else {
        VILA_TRY(gemm(y, C1, w->fc1_w, C1, w->fc1_b, nullptr, 0, mid, 3 * C, T, 3 * C, C1, EPI_GELU_ERF, s));
        VILA_TRY(launch_layernorm(mid, B(w->ln2_w), B(w->ln2_b), mid, T, 3 * C, 1e-5f, s));
        VILA_TRY(gemm(mid, 3 * C, w->fc2_w, 3 * C, w->fc2_b, nullptr, 0, h1, H, T, H, 3 * C, EPI_GELU_ERF, s));
        VILA_TRY(gemm(h1, H, w->fc3_w, H, w->fc3_b, nullptr, 0, out, H, T, H, H, EPI_NONE, s));
    }
    return 0;
}

// =================================================================================================
// Embedding / splice
// =================================================================================================
extern "C" int vila_embed_tokens(const void* table, int64_t vocab, int hidden, const int64_t* ids, int n, void* out, vila_stream_t stream) {
    return launch_embed_gather(B(table), ids, B(out), n, hidden, vocab, S(stream));
}
extern "C" int vila_copy_rows(const void* src, void* dst, const int32_t* src_row, const int32_t* dst_row, int n, int hidden, vila_stream_t stream) {
    return launch_copy_rows(B(src), B(dst), src_row, dst_row, n, hidden, S(stream));
}

// =================================================================================================
// LLM prefill
// =================================================================================================
// VILA_PREFILL_OPROJ_SPLITK=0: o_proj never takes the K-sliced path for the sake of the fused post-attention norm (A/B switch)
static bool prefill_oproj_norm();
static bool prefill_oproj_norm_env() {
    static int v = -1;
    if (v < 0) { const char* e = getenv("VILA_PREFILL_OPROJ_SPLITK"); v = (e && e[0] == '0') ? 0 : 1; }
    return v == 1;
}
// tuning / test hook (vila_hip_tuning.h): -1 = the environment's choice (default on), 0 / 1 = off / on
static int g_prefill_qkv_rope = -1, g_prefill_oproj_norm = -1;
extern "C" void vila_prefill_force_fusions(int qkv_rope, int oproj_norm) { g_prefill_qkv_rope = qkv_rope; g_prefill_oproj_norm = oproj_norm; }
static bool prefill_oproj_norm() { return g_prefill_oproj_norm >= 0 ? g_prefill_oproj_norm != 0 : prefill_oproj_norm_env(); }
static bool prefill_qkv_rope() {
    if (g_prefill_qkv_rope >= 0) return g_prefill_qkv_rope != 0;
    static int v = -1;
    if (v < 0) { const char* e = getenv("VILA_PREFILL_QKV_SPLITK"); v = (e && e[0] == '0') ? 0 : 1; }
    return v == 1;
}
extern "C" size_t vila_llm_prefill_workspace_bytes(const VilaLlmShape* s, int T) {
    const size_t H = s->hidden, F = s->inter, QKV = (size_t)(s->q_heads + 2 * s->kv_heads) * s->head_dim;
    size_t b = 0;
    b += 2 * align_up((size_t)T * H * 2, 256);                 // x, h
    b += align_up((size_t)T * QKV * 2, 256);                   // qkv
    b += align_up((size_t)T * F * 2, 256);                     // act
    b += 2 * align_up((size_t)T * (s->head_dim / 2) * 4, 256); // rope cos/sin
    b += align_up((size_t)(T > 8 ? T : 8) * H * 2, 256);       // gathered last rows / final norm (the pruned last layer keeps 2 x n_last <= 8 rows there)
    b += align_up((size_t)8 * T * H * 4, 256);                 // split-K fp32 slabs (down_proj: up to 8 slices; tail round of gate/up) at small T
    return b + 8192;
}
// the W4A16 GEMMs' K-slice slabs (gemm_w4.hip): the largest of the four projections' (the W4 prefill has them in place of the bf16 slabs)
static size_t prefill_w4_gemm_ws(const VilaLlmShape& sh, int T) {
    const int H = sh.hidden, F = sh.inter, QS = sh.q_heads * sh.head_dim, QKV = (sh.q_heads + 2 * sh.kv_heads) * sh.head_dim;
    size_t b = gemm_w4_workspace_bytes(T, QKV, H, 2);
    const size_t o = gemm_w4_workspace_bytes(T, H, QS, 0), gu = gemm_w4_workspace_bytes(T, F, H, 1), dn = gemm_w4_workspace_bytes(T, H, F, 0);
    if (o > b) b = o;
    if (gu > b) b = gu;
    if (dn > b) b = dn;
    return b;
}
extern "C" size_t vila_llm_prefill_w4_workspace_bytes(const VilaLlmShape* s, int T) {
    return vila_llm_prefill_workspace_bytes(s, T) + prefill_w4_gemm_ws(*s, T) + 256;
}

// One projection of a decoder layer for ONE row as a decode GEMV (the batch-1 decode step, the pruned last layer of the prefill): the bf16
// kernel on g (gemv.hip), or with int4 weights (w4) the W4A16 GEMV (gemv_w4.hip) on the same operands and epilogue.  bf16 mode 2 (x = the
// merge of the decode attention's 256-key partials) is W4 mode 4.
static int proj_gemv(const GemvArgs& g, bool w4, const void* wq, const void* wsz, hipStream_t s) {
    if (!w4) return launch_gemv(g, s);
    GemvW4Args a{};
    a.x = g.x; a.norm_w = g.norm_w; a.eps = g.eps; a.Wq = (const uint32_t*)wq; a.Wsz = (const uint32_t*)wsz; a.bias = g.bias; a.residual = g.residual;
    a.y = g.y; a.N = g.N; a.K = g.K; a.mode = g.mode == 2 ? 4 : g.mode;
    a.part_o = g.part_o; a.part_ml = g.part_ml; a.pos_ptr = g.pos_ptr; a.n_splits = g.n_splits; a.split_keys = g.split_keys;
    return launch_gemv_w4(a, s);
}

// The LLM prefill.  ql == nullptr: the bf16 projections, whose GEMMs may take the follow-up (RoPE + KV-cache scatter, the next RMSNorm) along
// in their split-K reduce and say so through rope_done / ln2_done / ln1_done.  ql != nullptr (vila_llm_prefill_w4): the five decoder
// projections read from the int4 layers (gemm_w4.hip), so a quantised model runs from its int4 weights alone; those GEMMs take no follow-up,
// so the standalone rmsnorm / rope_kv kernels run instead.
// ap != nullptr (vila_llm_prefill_append / _w4): the T tokens are ONE sequence continuing slot ap->slot of the cache at position ap->past.  The
// positions and the slot of every token are then made here (two int32 arrays at the end of the workspace) and the attention reads its keys and
// values from the slot (launch_attn_append) instead of the q/k/v buffer; everything else is the loop below as it stands.
struct PrefillAppend { int past, slot; };
static size_t prefill_append_extra(int T) { return 2 * align_up((size_t)T * 4, 256) + 512; }
extern "C" size_t vila_llm_prefill_append_workspace_bytes(const VilaLlmShape* s, int T) {
    return vila_llm_prefill_workspace_bytes(s, T) + prefill_append_extra(T);
}
extern "C" size_t vila_llm_prefill_append_w4_workspace_bytes(const VilaLlmShape* s, int T) {
    return vila_llm_prefill_w4_workspace_bytes(s, T) + prefill_append_extra(T);
}
static int llm_prefill_impl(const VilaLlmWeights* w, const VilaLlmLayerW4* ql, const void* embeds, const int32_t* positions,
                            const int32_t* cu_seqlens, int n_seq, int T, int max_seqlen, const int32_t* seq_of_tok, const VilaKvCache* cache,
                            const int32_t* last_rows, int n_last, float* last_logits, float* all_logits, void* final_hidden,
                            void* layer_hidden, void* workspace, size_t workspace_bytes, vila_stream_t stream, const PrefillAppend* ap = nullptr) {
    const VilaLlmShape& sh = w->shape;
    hipStream_t s = S(stream);
    const bool w4 = ql != nullptr;
    const char* fn = ap ? (w4 ? "llm_prefill_append_w4" : "llm_prefill_append") : (w4 ? "llm_prefill_w4" : "llm_prefill");
    VILA_REQUIRE(T > 0 && n_seq > 0, "%s: empty input", fn);
    VILA_REQUIRE(sh.q_heads % sh.kv_heads == 0, "llm: q heads must be a multiple of kv heads");
    VILA_REQUIRE(cu_seqlens != nullptr || n_seq == 1, "%s: n_seq > 1 needs cu_seqlens", fn);
    VILA_REQUIRE(workspace_bytes >= (w4 ? vila_llm_prefill_w4_workspace_bytes(&sh, T) : vila_llm_prefill_workspace_bytes(&sh, T)) + (ap ? prefill_append_extra(T) : 0),
                 "%s: workspace too small", fn);
    const int H = sh.hidden, F = sh.inter, hd = sh.head_dim, QS = sh.q_heads * hd, KS = sh.kv_heads * hd, QKV = QS + 2 * KS;
    VILA_REQUIRE(QS == H, "llm: q_heads*head_dim (%d) must equal hidden (%d) for the in-place attention buffer", QS, H);
    Arena a(workspace, workspace_bytes);
    bf16_t* x = a.take<bf16_t>((size_t)T * H);
    bf16_t* h = a.take<bf16_t>((size_t)T * H);
    bf16_t* qkv = a.take<bf16_t>((size_t)T * QKV);
    bf16_t* act = a.take<bf16_t>((size_t)T * F);
    float* cs = a.take<float>((size_t)T * hd / 2);
    float* sn = a.take<float>((size_t)T * hd / 2);
    bf16_t* lastbuf = a.take<bf16_t>((size_t)(T > 8 ? T : 8) * H);
    const size_t skws_bytes = w4 ? 0 : (size_t)8 * T * H * 4;       // the bf16 GEMMs' split-K fp32 slabs
    float* skws = w4 ? nullptr : a.take<float>(skws_bytes / 4);
    const size_t gws_bytes = w4 ? prefill_w4_gemm_ws(sh, T) : 0;     // the W4A16 GEMMs' slabs
    char* gws = w4 ? a.take<char>(gws_bytes) : nullptr;
    if (ap != nullptr) {
        int32_t* apos = a.take<int32_t>((size_t)T);
        int32_t* aseq = a.take<int32_t>((size_t)T);
        VILA_REQUIRE(a.ok(), "%s: workspace arena overflow", fn);
        VILA_TRY(launch_append_index(apos, aseq, ap->past, ap->slot, T, s));
        positions = apos; seq_of_tok = aseq;
    }
    VILA_REQUIRE(a.ok(), "%s: workspace arena overflow", fn);
    if (cache != nullptr) VILA_REQUIRE(max_seqlen <= cache->max_ctx, "%s: sequence (%d) longer than the KV cache (%d)", fn, max_seqlen, cache->max_ctx);

    VILA_HIP(hipMemcpyAsync(x, embeds, (size_t)T * H * 2, hipMemcpyDeviceToDevice, s));
    VILA_TRY(launch_rope_table(positions, cs, sn, T, hd, sh.rope_theta, s));
    bf16_t* taps = B(layer_hidden);
    if (taps) VILA_HIP(hipMemcpyAsync(taps, x, (size_t)T * H * 2, hipMemcpyDeviceToDevice, s));

    // only last-row logits wanted (generation): the last layer is finished for those rows alone (see below)
    const bool prune_last = final_hidden == nullptr && all_logits == nullptr && taps == nullptr && cache != nullptr && last_logits != nullptr &&
                            last_rows != nullptr && n_last >= 1 && n_last <= 4 && H % 8 == 0 && F % 8 == 0;
    auto gemm4 = [&](const bf16_t* xin, const void* q, const void* sz, const void* bias, const bf16_t* res, bf16_t* y, int N, int K, int mode) {
        GemmW4Args g{};
        g.x = xin; g.Wq = (const uint32_t*)q; g.Wsz = (const uint32_t*)sz; g.bias = B(bias); g.residual = res; g.y = y;
        g.M = T; g.N = N; g.K = K; g.mode = mode; g.n_rope_heads = sh.q_heads + sh.kv_heads; g.hd = hd;
        return launch_gemm_w4(g, gws, gws_bytes, s);
    };
    int ln1_done = 0;                                           // the previous layer's down-proj reduce already wrote input_layernorm(x) into h
    for (int l = 0; l < sh.n_layers; ++l) {
        const VilaLlmLayer& L = w->layers[l];
        const VilaLlmLayerW4 Q = w4 ? ql[l] : VilaLlmLayerW4{};
        if (w4) VILA_REQUIRE(L.bq != nullptr && B(L.bk) == B(L.bq) + QS && B(L.bv) == B(L.bk) + KS,
                             "llm_prefill_w4: the q/k/v biases must be one contiguous q|k|v vector (layer %d)", l);
        if (!ln1_done) VILA_TRY(launch_rmsnorm(x, B(L.ln1_w), h, T, H, sh.rms_eps, s));
        ln1_done = 0;
        bf16_t* kc = nullptr; bf16_t* vc = nullptr; int max_ctx = 0;
        if (cache != nullptr) {
            const size_t per_layer = (size_t)cache->n_slots * sh.kv_heads * cache->max_ctx * hd;
            kc = B(cache->k) + l * per_layer; vc = B(cache->v) + l * per_layer; max_ctx = cache->max_ctx;
        }
        int rope_done = 0;
        if (w4) {
            VILA_TRY(gemm4(h, Q.qkv_q, Q.qkv_sz, L.bq, nullptr, qkv, QKV, H, 2));                 // q | k | v + bias, natural column order
        } else if (qkv_fused(L.wq, L.wk, L.wv, L.bq, L.bk, L.bv, QS, KS, H)) {
            // one GEMM for q | k | v; where its grid is K-sliced (S = 769: 54 tiles x 4 slices) the reduce adds the bias, rotates q and k and
            // writes K / V into the cache (VILA_PREFILL_QKV_SPLITK=0: ring GEMM + rope_kv_kernel as in rounds 1-5)
            NextRope nr;
            nr.cs = cs; nr.sn = sn; nr.pos = positions; nr.seq = seq_of_tok; nr.kc = kc; nr.vc = vc; nr.nq = sh.q_heads; nr.nkv = sh.kv_heads; nr.hd = hd;
            nr.max_ctx = max_ctx; nr.done = &rope_done;
            VILA_TRY(gemm(h, H, L.wq, H, L.bq, nullptr, 0, qkv, QKV, T, QKV, H, EPI_NONE, s, nullptr, 0, skws, skws_bytes, 0, nullptr, prefill_qkv_rope() ? &nr : nullptr));
        } else {
            VILA_TRY(gemm(h, H, L.wq, H, L.bq, nullptr, 0, qkv, QKV, T, QS, H, EPI_NONE, s));
            VILA_TRY(gemm(h, H, L.wk, H, L.bk, nullptr, 0, qkv + QS, QKV, T, KS, H, EPI_NONE, s));
            VILA_TRY(gemm(h, H, L.wv, H, L.bv, nullptr, 0, qkv + QS + KS, QKV, T, KS, H, EPI_NONE, s));
        }
        if (!rope_done) VILA_TRY(launch_rope_kv(qkv, cs, sn, positions, seq_of_tok, kc, vc, T, sh.q_heads, sh.kv_heads, hd, max_ctx, s));
        AttnArgs at{};
        at.q = qkv; at.k = qkv + QS; at.v = qkv + QS + KS; at.o = h;
        at.q_tok_stride = at.k_tok_stride = at.v_tok_stride = QKV; at.o_tok_stride = QS;
        at.q_head_stride = at.k_head_stride = at.v_head_stride = at.o_head_stride = hd;
        at.cu_seqlens = cu_seqlens; at.n_seq = n_seq; at.total_tokens = T; at.max_seqlen = (cu_seqlens ? max_seqlen : T);
        at.n_q_heads = sh.q_heads; at.n_kv_heads = sh.kv_heads; at.head_dim = hd; at.causal = 1;
        at.scale = 1.0f / sqrtf((float)hd); at.lse = nullptr;
        if (ap != nullptr) {
            const size_t slot_off = (size_t)ap->slot * sh.kv_heads * max_ctx * hd;
            VILA_TRY(launch_attn_append(qkv, QKV, kc + slot_off, vc + slot_off, ap->past, T, h, QS, sh.q_heads, sh.kv_heads, max_ctx, at.scale, s));
        } else {
            VILA_TRY(launch_attn_fwd(at, s));
        }
        if (l == sh.n_layers - 1 && prune_last) {
            // Generation prefill: after the last layer's K / V are in the cache only the rows whose logits are asked for feed anything.
            // Their o_proj, post-attention norm and MLP run as three decode GEMVs per row (weights stream once at HBM rate) instead of
            // four GEMMs over all T rows: the same kernels and arithmetic order per row as the decode step, which is parity-tested against this path.
            VILA_TRY(launch_copy_rows(h, lastbuf, last_rows, nullptr, n_last, QS, s));             // attention output rows
            VILA_TRY(launch_copy_rows(x, lastbuf + (size_t)n_last * H, last_rows, nullptr, n_last, H, s));   // residual rows
            for (int r = 0; r < n_last; ++r) {
                bf16_t* ar = lastbuf + (size_t)r * H;                       // attention row  -> later the row's final hidden state
                bf16_t* xr = lastbuf + (size_t)(n_last + r) * H;            // residual row
                bf16_t* fr = act + (size_t)r * F;                           // silu(gate) * up of the row
                GemvArgs g0{};
                g0.x = ar; g0.W = B(L.wo); g0.residual = xr; g0.y = xr; g0.N = H; g0.K = QS; g0.mode = 0;
                VILA_TRY(proj_gemv(g0, w4, Q.o_q, Q.o_sz, s));
                GemvArgs g1{};
                g1.x = xr; g1.norm_w = B(L.ln2_w); g1.eps = sh.rms_eps; g1.W = B(L.w_gate); g1.W2 = B(L.w_up); g1.y = fr; g1.N = F; g1.K = H; g1.mode = 1;
                VILA_TRY(proj_gemv(g1, w4, Q.gateup_q, Q.gateup_sz, s));
                GemvArgs g2{};
                g2.x = fr; g2.W = B(L.w_down); g2.residual = xr; g2.y = ar; g2.N = H; g2.K = F; g2.mode = 0;
                VILA_TRY(proj_gemv(g2, w4, Q.down_q, Q.down_sz, s));
            }
            break;
        }
        // x += o_proj(attn).  The post-attention RMSNorm is offered to the bf16 GEMM: where its grid is K-sliced (S = 769: 42 tiles x 6 slices)
        // the reduce holds whole rows and writes h = norm(x) as well (h is free: the GEMM kernel that read it has finished when the reduce runs)
        int ln2_done = 0;
        if (w4) {
            VILA_TRY(gemm4(h, Q.o_q, Q.o_sz, nullptr, x, x, H, QS, 0));
        } else {
            NextNorm n2;
            n2.w = L.ln2_w; n2.eps = sh.rms_eps; n2.rms = 1; n2.out = h; n2.done = &ln2_done;
            VILA_TRY(gemm(h, QS, L.wo, QS, nullptr, x, H, x, H, T, H, QS, EPI_NONE, s, nullptr, 0, skws, skws_bytes, 0, prefill_oproj_norm() ? &n2 : nullptr));
        }
        if (!ln2_done) VILA_TRY(launch_rmsnorm(x, B(L.ln2_w), h, T, H, sh.rms_eps, s));
        // MLP: silu(gate) * up, then x += down(...); where the bf16 down GEMM is K-sliced (S = 769: 56 tiles cannot fill the chip) its reduce takes
        // the NEXT layer's input_layernorm along (h is free: gate/up has consumed it)
        if (w4) {
            VILA_TRY(gemm4(h, Q.gateup_q, Q.gateup_sz, nullptr, nullptr, act, F, H, 1));
            VILA_TRY(gemm4(act, Q.down_q, Q.down_sz, nullptr, x, x, H, F, 0));
        } else {
            VILA_TRY(gemm(h, H, L.w_gate, H, nullptr, nullptr, 0, act, F, T, F, H, EPI_GATEUP, s, L.w_up, 0, skws, skws_bytes));
            NextNorm nn;
            const bool offer = l + 1 < sh.n_layers;
            if (offer) { nn.w = w->layers[l + 1].ln1_w; nn.eps = sh.rms_eps; nn.rms = 1; nn.out = h; nn.done = &ln1_done; }
            VILA_TRY(gemm(act, F, L.w_down, F, nullptr, x, H, x, H, T, H, F, EPI_NONE, s, nullptr, 0, skws, skws_bytes, 0, offer ? &nn : nullptr));
        }
        if (taps) VILA_HIP(hipMemcpyAsync(taps + (size_t)(l + 1) * T * H, x, (size_t)T * H * 2, hipMemcpyDeviceToDevice, s));
    }

    if (final_hidden != nullptr || all_logits != nullptr) {
        bf16_t* fh = final_hidden ? B(final_hidden) : h;
        VILA_TRY(launch_rmsnorm(x, B(w->norm_w), fh, T, H, sh.rms_eps, s));
        if (all_logits) VILA_TRY(gemm(fh, H, w->lm_head, H, nullptr, nullptr, 0, all_logits, sh.vocab, T, sh.vocab, H, EPI_NONE, s, nullptr, 1));
    }
    if (n_last > 0 && last_logits != nullptr) {
        VILA_REQUIRE(last_rows != nullptr, "%s: last_rows is NULL", fn);
        if (!prune_last) VILA_TRY(launch_copy_rows(x, lastbuf, last_rows, nullptr, n_last, H, s));     // (pruned: lastbuf already holds the rows)
        if (n_last == 1) {
            GemvArgs g{};
            g.x = lastbuf; g.norm_w = B(w->norm_w); g.eps = sh.rms_eps; g.W = B(w->lm_head); g.y_f32 = last_logits;
            g.N = sh.vocab; g.K = H; g.mode = 0;
            VILA_TRY(launch_gemv(g, s));
        } else {
            VILA_TRY(launch_rmsnorm(lastbuf, B(w->norm_w), lastbuf, n_last, H, sh.rms_eps, s));
            VILA_TRY(gemm(lastbuf, H, w->lm_head, H, nullptr, nullptr, 0, last_logits, sh.vocab, n_last, sh.vocab, H, EPI_NONE, s, nullptr, 1));
        }
    }
    return 0;
}
extern "C" int vila_llm_prefill(const VilaLlmWeights* w, const void* embeds, const int32_t* positions, const int32_t* cu_seqlens,
                                int n_seq, int T, int max_seqlen, const int32_t* seq_of_tok, const VilaKvCache* cache,
                                const int32_t* last_rows, int n_last, float* last_logits, float* all_logits, void* final_hidden,
                                void* layer_hidden, void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    return llm_prefill_impl(w, nullptr, embeds, positions, cu_seqlens, n_seq, T, max_seqlen, seq_of_tok, cache, last_rows, n_last, last_logits,
                            all_logits, final_hidden, layer_hidden, workspace, workspace_bytes, stream);
}
// the prefill with the five decoder projections read from the int4 layers; embed, norms, the fused q|k|v biases and the bf16 lm_head come from `w`
extern "C" int vila_llm_prefill_w4(const VilaLlmWeights* w, const VilaLlmLayerW4* ql, const void* embeds, const int32_t* positions,
                                   const int32_t* cu_seqlens, int n_seq, int T, int max_seqlen, const int32_t* seq_of_tok, const VilaKvCache* cache,
                                   const int32_t* last_rows, int n_last, float* last_logits, float* all_logits, void* final_hidden,
                                   void* layer_hidden, void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    VILA_REQUIRE(ql != nullptr, "llm_prefill_w4: the int4 layers are NULL");
    return llm_prefill_impl(w, ql, embeds, positions, cu_seqlens, n_seq, T, max_seqlen, seq_of_tok, cache, last_rows, n_last, last_logits,
                            all_logits, final_hidden, layer_hidden, workspace, workspace_bytes, stream);
}

// The prefill under ONE LoRA adapter (a request admitted under an adapter of the serving bank): llm_prefill_impl's sibling from launches that exist.  Per
// projection the trainer's forward dataflow (vila_amd/lora.py): t = lora_down(stack input, A), u = lora_up(t slice, Bt, scale, res = the linear's
// residual), y = gemm(input, W, bias, residual = u).  The GEMMs take no follow-up along, so RoPE + cache scatter and the norms are their own launches;
// gate and up are two GEMMs and silu_mul; every row runs every layer.
extern "C" size_t vila_llm_prefill_lora_workspace_bytes(const VilaLlmShape* s, int T, int r) {
    const size_t F = s->inter, QKV = (size_t)(s->q_heads + 2 * s->kv_heads) * s->head_dim, wide = QKV > F ? QKV : F;
    const size_t down = vila_lora_down_workspace_bytes(T, (int)(F > (size_t)s->hidden ? F : (size_t)s->hidden), 3 * r);
    return vila_llm_prefill_workspace_bytes(s, T) + align_up((size_t)T * 3 * r * 2, 256) + align_up((size_t)T * wide * 2, 256) + align_up((size_t)T * F * 2, 256) +
           align_up(down, 256) + 1024;
}
extern "C" int vila_llm_prefill_lora(const VilaLlmWeights* w, const VilaLoraLayer* lora, int r, float scale, const void* embeds, const int32_t* positions,
                                     const int32_t* cu_seqlens, int n_seq, int T, int max_seqlen, const int32_t* seq_of_tok, const VilaKvCache* cache,
                                     const int32_t* last_rows, int n_last, float* last_logits, float* all_logits, void* final_hidden, void* workspace,
                                     size_t workspace_bytes, vila_stream_t stream) {
    const char* fn = "llm_prefill_lora";
    VILA_REQUIRE(w != nullptr && lora != nullptr && embeds != nullptr && positions != nullptr && workspace != nullptr, "%s: NULL argument", fn);
    const VilaLlmShape& sh = w->shape;
    hipStream_t s = S(stream);
    VILA_REQUIRE(T > 0 && n_seq > 0, "%s: empty input", fn);
    VILA_REQUIRE(r == 16 || r == 32 || r == 48 || r == 64, "%s: rank 16, 32, 48 or 64 (got %d)", fn, r);
    VILA_REQUIRE(sh.q_heads % sh.kv_heads == 0, "llm: q heads must be a multiple of kv heads");
    VILA_REQUIRE(cu_seqlens != nullptr || n_seq == 1, "%s: n_seq > 1 needs cu_seqlens", fn);
    VILA_REQUIRE(workspace_bytes >= vila_llm_prefill_lora_workspace_bytes(&sh, T, r), "%s: workspace too small", fn);
    const int H = sh.hidden, F = sh.inter, hd = sh.head_dim, QS = sh.q_heads * hd, KS = sh.kv_heads * hd, QKV = QS + 2 * KS;
    VILA_REQUIRE(QS == H, "llm: q_heads*head_dim (%d) must equal hidden (%d) for the in-place attention buffer", QS, H);
    VILA_REQUIRE(H % 8 == 0 && F % 8 == 0 && KS % 8 == 0, "%s: hidden, intermediate and kv widths must be multiples of 8", fn);
    Arena a(workspace, workspace_bytes);
    bf16_t* x = a.take<bf16_t>((size_t)T * H);
    bf16_t* h = a.take<bf16_t>((size_t)T * H);
    bf16_t* qkv = a.take<bf16_t>((size_t)T * QKV);
    bf16_t* act = a.take<bf16_t>((size_t)T * F);
    float* cs = a.take<float>((size_t)T * hd / 2);
    float* sn = a.take<float>((size_t)T * hd / 2);
    bf16_t* lastbuf = a.take<bf16_t>((size_t)(T > 8 ? T : 8) * H);
    const size_t skws_bytes = (size_t)8 * T * H * 4;
    float* skws = a.take<float>(skws_bytes / 4);
    bf16_t* t = a.take<bf16_t>((size_t)T * 3 * r);                     // x . A^T of the current stack
    bf16_t* u = a.take<bf16_t>((size_t)T * (QKV > F ? QKV : F));         // scale * t . Bt (+ the residual): the base GEMM's residual
    bf16_t* gate = a.take<bf16_t>((size_t)T * F);
    const size_t dws_bytes = vila_lora_down_workspace_bytes(T, F > H ? F : H, 3 * r);
    char* dws = a.take<char>(dws_bytes);
    VILA_REQUIRE(a.ok(), "%s: workspace arena overflow", fn);
    if (cache != nullptr) VILA_REQUIRE(max_seqlen <= cache->max_ctx, "%s: sequence (%d) longer than the KV cache (%d)", fn, max_seqlen, cache->max_ctx);
    auto down = [&](const bf16_t* in, int K, const void* A, int Rs) {
        return vila_lora_down_bf16(in, K, A, K, t, 3 * r, T, K, Rs, 1.0f, dws, dws_bytes, stream);
    };
    // member j of the stack: columns [c0, c0 + N) of the stack's Ntot; res (nullable, row stride H) is the linear's residual
    auto up = [&](int j, const void* Bt, int Ntot, int c0, int N, const bf16_t* res, bf16_t* out, int ldo) {
        return vila_lora_up_bf16(t + j * r, 3 * r, B(Bt) + c0, Ntot, res, H, out, ldo, T, N, r, scale, nullptr, 0, stream);
    };

    VILA_HIP(hipMemcpyAsync(x, embeds, (size_t)T * H * 2, hipMemcpyDeviceToDevice, s));
    VILA_TRY(launch_rope_table(positions, cs, sn, T, hd, sh.rope_theta, s));
    for (int l = 0; l < sh.n_layers; ++l) {
        const VilaLlmLayer& L = w->layers[l];
        const VilaLoraLayer& A = lora[l];
        VILA_REQUIRE(A.a_qkv && A.bt_qkv && A.a_o && A.bt_o && A.a_gateup && A.bt_gateup && A.a_down && A.bt_down, "%s: adapter layer %d has a NULL buffer", fn, l);
        VILA_REQUIRE(qkv_fused(L.wq, L.wk, L.wv, L.bq, L.bk, L.bv, QS, KS, H), "%s: q/k/v projection weights and biases must be views of one fused buffer", fn);
        VILA_TRY(launch_rmsnorm(x, B(L.ln1_w), h, T, H, sh.rms_eps, s));
        bf16_t* kc = nullptr; bf16_t* vc = nullptr; int max_ctx = 0;
        if (cache != nullptr) {
            const size_t per_layer = (size_t)cache->n_slots * sh.kv_heads * cache->max_ctx * hd;
            kc = B(cache->k) + l * per_layer; vc = B(cache->v) + l * per_layer; max_ctx = cache->max_ctx;
        }
        VILA_TRY(down(h, H, A.a_qkv, 3 * r));
        VILA_TRY(up(0, A.bt_qkv, QKV, 0, QS, nullptr, u, QKV));
        VILA_TRY(up(1, A.bt_qkv, QKV, QS, KS, nullptr, u + QS, QKV));
        VILA_TRY(up(2, A.bt_qkv, QKV, QS + KS, KS, nullptr, u + QS + KS, QKV));
        VILA_TRY(gemm(h, H, L.wq, H, L.bq, u, QKV, qkv, QKV, T, QKV, H, EPI_NONE, s));
        VILA_TRY(launch_rope_kv(qkv, cs, sn, positions, seq_of_tok, kc, vc, T, sh.q_heads, sh.kv_heads, hd, max_ctx, s));
        AttnArgs at{};
        at.q = qkv; at.k = qkv + QS; at.v = qkv + QS + KS; at.o = h;
        at.q_tok_stride = at.k_tok_stride = at.v_tok_stride = QKV; at.o_tok_stride = QS;
        at.q_head_stride = at.k_head_stride = at.v_head_stride = at.o_head_stride = hd;
        at.cu_seqlens = cu_seqlens; at.n_seq = n_seq; at.total_tokens = T; at.max_seqlen = (cu_seqlens ? max_seqlen : T);
        at.n_q_heads = sh.q_heads; at.n_kv_heads = sh.kv_heads; at.head_dim = hd; at.causal = 1;
        at.scale = 1.0f / sqrtf((float)hd); at.lse = nullptr;
        VILA_TRY(launch_attn_fwd(at, s));
        VILA_TRY(down(h, QS, A.a_o, r));                                                          // x += o_proj(attn): u = x + s t Bt, x = gemm + u
        VILA_TRY(up(0, A.bt_o, H, 0, H, x, u, H));
        VILA_TRY(gemm(h, QS, L.wo, QS, nullptr, u, H, x, H, T, H, QS, EPI_NONE, s, nullptr, 0, skws, skws_bytes));
        VILA_TRY(launch_rmsnorm(x, B(L.ln2_w), h, T, H, sh.rms_eps, s));
        VILA_TRY(down(h, H, A.a_gateup, 2 * r));
        VILA_TRY(up(0, A.bt_gateup, 2 * F, 0, F, nullptr, u, F));
        VILA_TRY(gemm(h, H, L.w_gate, H, nullptr, u, F, gate, F, T, F, H, EPI_NONE, s, nullptr, 0, skws, skws_bytes));
        VILA_TRY(up(1, A.bt_gateup, 2 * F, F, F, nullptr, u, F));
        VILA_TRY(gemm(h, H, L.w_up, H, nullptr, u, F, u, F, T, F, H, EPI_NONE, s, nullptr, 0, skws, skws_bytes));
        VILA_TRY(launch_silu_mul_fwd(gate, u, act, (int64_t)T * F, s));
        VILA_TRY(down(act, F, A.a_down, r));
        VILA_TRY(up(0, A.bt_down, H, 0, H, x, u, H));
        VILA_TRY(gemm(act, F, L.w_down, F, nullptr, u, H, x, H, T, H, F, EPI_NONE, s, nullptr, 0, skws, skws_bytes));
    }
    if (final_hidden != nullptr || all_logits != nullptr) {
        bf16_t* fh = final_hidden ? B(final_hidden) : h;
        VILA_TRY(launch_rmsnorm(x, B(w->norm_w), fh, T, H, sh.rms_eps, s));
        if (all_logits) VILA_TRY(gemm(fh, H, w->lm_head, H, nullptr, nullptr, 0, all_logits, sh.vocab, T, sh.vocab, H, EPI_NONE, s, nullptr, 1));
    }
    if (n_last > 0 && last_logits != nullptr) {
        VILA_REQUIRE(last_rows != nullptr, "%s: last_rows is NULL", fn);
        VILA_TRY(launch_copy_rows(x, lastbuf, last_rows, nullptr, n_last, H, s));
        VILA_TRY(launch_rmsnorm(lastbuf, B(w->norm_w), lastbuf, n_last, H, sh.rms_eps, s));
        VILA_TRY(gemm(lastbuf, H, w->lm_head, H, nullptr, nullptr, 0, last_logits, sh.vocab, n_last, sh.vocab, H, EPI_NONE, s, nullptr, 1));
    }
    return 0;
}

// The append prefill: T tokens of ONE sequence continue slot `slot` of the cache, which holds `past` positions.
static int llm_prefill_append(const VilaLlmWeights* w, const VilaLlmLayerW4* ql, const void* embeds, int T, int past, int slot, const VilaKvCache* cache,
                              const int32_t* last_rows, int n_last, float* last_logits, void* final_hidden, void* layer_hidden, void* workspace,
                              size_t workspace_bytes, vila_stream_t stream) {
    const char* fn = ql ? "llm_prefill_append_w4" : "llm_prefill_append";
    VILA_REQUIRE(w != nullptr && embeds != nullptr && cache != nullptr && cache->k != nullptr && cache->v != nullptr, "%s: weights, embeds and cache must be given", fn);
    const VilaLlmShape& sh = w->shape;
    VILA_REQUIRE(T >= 1 && past >= 0, "%s: T (%d) must be >= 1 and past (%d) >= 0", fn, T, past);
    VILA_REQUIRE((int64_t)past + T <= cache->max_ctx, "%s: past + T (%d + %d) exceeds the KV cache (%d positions)", fn, past, T, cache->max_ctx);
    VILA_REQUIRE(slot >= 0 && slot < cache->n_slots, "%s: slot %d outside the cache's %d slots", fn, slot, cache->n_slots);
    VILA_REQUIRE(sh.head_dim == 128, "%s: head_dim 128 only (got %d)", fn, sh.head_dim);
    VILA_REQUIRE(sh.q_heads * sh.head_dim == sh.hidden, "%s: q_heads*head_dim (%d) must equal hidden (%d)", fn, sh.q_heads * sh.head_dim, sh.hidden);
    const PrefillAppend ap{past, slot};
    return llm_prefill_impl(w, ql, embeds, nullptr, nullptr, 1, T, T, nullptr, cache, last_rows, n_last, last_logits, nullptr, final_hidden, layer_hidden,
                            workspace, workspace_bytes, stream, &ap);
}
extern "C" int vila_llm_prefill_append(const VilaLlmWeights* w, const void* embeds, int T, int past, int slot, const VilaKvCache* cache,
                                       const int32_t* last_rows, int n_last, float* last_logits, void* final_hidden, void* layer_hidden,
                                       void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    return llm_prefill_append(w, nullptr, embeds, T, past, slot, cache, last_rows, n_last, last_logits, final_hidden, layer_hidden, workspace,
                              workspace_bytes, stream);
}
extern "C" int vila_llm_prefill_append_w4(const VilaLlmWeights* w, const VilaLlmLayerW4* ql, const void* embeds, int T, int past, int slot,
                                          const VilaKvCache* cache, const int32_t* last_rows, int n_last, float* last_logits, void* final_hidden,
                                          void* layer_hidden, void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    VILA_REQUIRE(ql != nullptr, "llm_prefill_append_w4: the int4 layers are NULL");
    return llm_prefill_append(w, ql, embeds, T, past, slot, cache, last_rows, n_last, last_logits, final_hidden, layer_hidden, workspace,
                              workspace_bytes, stream);
}

// =================================================================================================
// LLM decode step (batch 1)
// =================================================================================================
static inline int dec_splits(int max_ctx) { return cdiv(max_ctx, DEC_KS); }
// kernel launches of one vila_llm_decode_step: prologue + per layer {qkv, attention (1 launch up to DEC_SHORT_CTX cached positions, else
// split-KV + merge), o_proj, gate/up, down} + lm_head (which also reduces each block's logits to one (max, index) pair) + the final pick, which
// advances the state as well
extern "C" int vila_llm_decode_launches(const VilaLlmShape* s, int max_ctx) {
    return 1 + s->n_layers * (max_ctx <= DEC_SHORT_CTX ? 5 : 6) + 2;      // a sampled step: + 3 (three selection launches and the advance after lm_head)
}
extern "C" size_t vila_llm_decode_workspace_bytes(const VilaLlmShape* s, int max_ctx) {
    const size_t H = s->hidden, F = s->inter, QS = (size_t)s->q_heads * s->head_dim;
    const size_t ns = dec_splits(max_ctx);
    size_t b = 0;
    b += 2 * align_up(H * 2, 256) + 2 * align_up(QS * 2, 256) + align_up(F * 2, 256);
    b += align_up(ns * QS * 4, 256) + align_up(ns * s->q_heads * 2 * 4, 256);
    b += 2 * align_up((size_t)gemv_grid_blocks(s->vocab) * 4, 256) + align_up((size_t)s->head_dim * 4, 256);
    b += align_up(QS * 2, 256);
    b += align_up(sample_workspace_bytes(), 256);
    return b + 4096;
}

// decode attention variant (vila_decode_force_attn): 1 or 2 (default) = per-head blocks over 256-key slices, merged in the prologue of the o_proj GEMV
// (8 waves per CU; until the GEMVs went to one block per CU, 1 meant 256 o_proj blocks and 2 meant 512); 0 = one block per query head over the whole
// context + plain o_proj (round 1).  Measured at context 785..913 (bench.py): 328.7 / 335.7 / 342.0 tok/s for 0 / 256 blocks / 512 blocks.
static int g_decode_attn = -1;     // -1: not set yet -> environment VILA_DECODE_ATTN, else 2
extern "C" void vila_decode_force_attn(int mode) { g_decode_attn = mode; }
static int decode_attn_mode() {
    if (g_decode_attn < 0) { const char* e = getenv("VILA_DECODE_ATTN"); g_decode_attn = (e && e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : 2; }
    return g_decode_attn;
}
static int decode_step_impl(const VilaLlmWeights* w, const VilaLlmLayerW4* ql, const VilaKvCache* cache, const VilaDecodeState* st,
                            void* workspace, size_t workspace_bytes, const VilaSampling* sp, vila_stream_t stream, const VilaPenalties* pen = nullptr,
                            const VilaConstraints* con = nullptr);
extern "C" int vila_llm_decode_step(const VilaLlmWeights* w, const VilaKvCache* cache, const VilaDecodeState* st,
                                    void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    return decode_step_impl(w, nullptr, cache, st, workspace, workspace_bytes, nullptr, stream);
}
// the same step with a stochastic pick (temperature / top-k / top-p) instead of argmax: generate(do_sample=True)
extern "C" int vila_llm_decode_step_sample(const VilaLlmWeights* w, const VilaKvCache* cache, const VilaDecodeState* st,
                                           void* workspace, size_t workspace_bytes, const VilaSampling* sp, vila_stream_t stream) {
    VILA_REQUIRE(sp != nullptr, "llm_decode_sample: sampling parameters are NULL");
    return decode_step_impl(w, nullptr, cache, st, workspace, workspace_bytes, sp, stream);
}
// W4A16 decode: the step with the five decoder-layer projections read from int4 group-128 weights, bf16 everything else
extern "C" int vila_llm_decode_step_w4(const VilaLlmWeights* w, const VilaLlmLayerW4* ql, const VilaKvCache* cache, const VilaDecodeState* st,
                                       void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    VILA_REQUIRE(ql != nullptr, "llm_decode_w4: the int4 layers are NULL");
    return decode_step_impl(w, ql, cache, st, workspace, workspace_bytes, nullptr, stream);
}
// the W4A16 step with a stochastic pick (generate(do_sample=True) on a quantised decoder)
extern "C" int vila_llm_decode_step_w4_sample(const VilaLlmWeights* w, const VilaLlmLayerW4* ql, const VilaKvCache* cache, const VilaDecodeState* st,
                                              void* workspace, size_t workspace_bytes, const VilaSampling* sp, vila_stream_t stream) {
    VILA_REQUIRE(sp != nullptr, "llm_decode_w4_sample: sampling parameters are NULL");
    VILA_REQUIRE(ql != nullptr, "llm_decode_w4: the int4 layers are NULL");
    return decode_step_impl(w, ql, cache, st, workspace, workspace_bytes, sp, stream);
}
// The penalised batch-1 step (penalty.hip): ql and sp nullable — bf16 / W4, greedy / sampled in one entry.
static int penalties_ok(const VilaPenalties* pen, int vocab, const char* fn) {
    VILA_REQUIRE(pen != nullptr && pen->repetition != nullptr && pen->presence != nullptr && pen->frequency != nullptr && pen->counts != nullptr,
                 "%s: the penalties or one of their arrays are NULL", fn);
    VILA_REQUIRE(pen->ld_counts >= vocab, "%s: the count rows (%lld apart) are shorter than the vocabulary %d", fn, (long long)pen->ld_counts, vocab);
    return 0;
}
extern "C" size_t vila_llm_decode_penalized_workspace_bytes(const VilaLlmShape* s, int max_ctx) {
    return align_up(vila_llm_decode_workspace_bytes(s, max_ctx), 256) + align_up((size_t)s->vocab * 4, 256) + 2 * align_up((size_t)PEN_SOLO_SLICES * 4, 256) + 256;
}
extern "C" int vila_llm_decode_step_penalized(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const VilaKvCache* cache, const VilaDecodeState* st,
                                              void* workspace, size_t workspace_bytes, const VilaSampling* sp, const VilaPenalties* pen, vila_stream_t stream) {
    VILA_REQUIRE(w != nullptr, "llm_decode_penalized: the weights are NULL");
    VILA_TRY(penalties_ok(pen, w->shape.vocab, "llm_decode_penalized"));
    return decode_step_impl(w, qlayers, cache, st, workspace, workspace_bytes, sp, stream, pen);
}
extern "C" int vila_logits_penalize_slices(void) { return PEN_PICK_SLICES; }
extern "C" int vila_logits_penalize_f32(const float* logits, int64_t ld, int n, int vocab, const VilaPenalties* pen, const int64_t* token, float* out,
                                        int64_t ld_out, float* pick_v, int* pick_i, vila_stream_t stream) {
    VILA_REQUIRE(pen != nullptr, "logits_penalize: the penalties are NULL");
    const Penalties P{pen->repetition, pen->presence, pen->frequency, pen->counts, pen->ld_counts};
    return launch_penalize(logits, ld, n, vocab, P, token, out, ld_out, PEN_PICK_SLICES, pick_v, pick_i, S(stream));
}
// Structured output (constrain.hip): the operator, and the batch-1 step with it between the (optional) penalties and the pick.
static int constraints_ok(const VilaConstraints* con, int vocab, const char* fn) {
    VILA_REQUIRE(con != nullptr && con->state != nullptr && con->cls != nullptr && con->next != nullptr && con->n_classes != nullptr,
                 "%s: the constraints or one of their arrays are NULL", fn);
    VILA_REQUIRE(con->ld_cls >= vocab, "%s: the class rows (%lld apart) are shorter than the vocabulary %d", fn, (long long)con->ld_cls, vocab);
    VILA_REQUIRE(con->ld_next >= 1, "%s: the table rows are %lld entries apart", fn, (long long)con->ld_next);
    return 0;
}
extern "C" int vila_logits_constrain_slices(void) { return PEN_PICK_SLICES; }
extern "C" int vila_logits_constrain_max_classes(void) { return CON_MAX_CLASSES; }
extern "C" int vila_logits_constrain_f32(const float* logits, int64_t ld, int n, int vocab, const VilaConstraints* con, const int64_t* token, float* out,
                                         int64_t ld_out, float* pick_v, int* pick_i, vila_stream_t stream) {
    VILA_REQUIRE(logits != nullptr && out != nullptr, "logits_constrain: NULL argument");
    VILA_REQUIRE(n >= 1 && n <= 65535 && vocab >= 1, "logits_constrain: 1..65535 rows of a non-empty vocabulary (got %d x %d)", n, vocab);
    VILA_TRY(constraints_ok(con, vocab, "logits_constrain"));
    const Constraints Cn{con->state, con->cls, con->ld_cls, con->next, con->ld_next, con->n_classes};
    return launch_constrain(logits, ld, n, vocab, Cn, token, out, ld_out, PEN_PICK_SLICES, pick_v, pick_i, S(stream));
}
extern "C" size_t vila_llm_decode_constrained_workspace_bytes(const VilaLlmShape* s, int max_ctx) { return vila_llm_decode_penalized_workspace_bytes(s, max_ctx); }
extern "C" int vila_llm_decode_step_constrained(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const VilaKvCache* cache, const VilaDecodeState* st,
                                                void* workspace, size_t workspace_bytes, const VilaSampling* sp, const VilaPenalties* pen,
                                                const VilaConstraints* con, vila_stream_t stream) {
    VILA_REQUIRE(w != nullptr, "llm_decode_constrained: the weights are NULL");
    if (pen != nullptr) VILA_TRY(penalties_ok(pen, w->shape.vocab, "llm_decode_constrained"));
    VILA_TRY(constraints_ok(con, w->shape.vocab, "llm_decode_constrained"));
    return decode_step_impl(w, qlayers, cache, st, workspace, workspace_bytes, sp, stream, pen, con);
}
// log-probabilities of the chosen token and its top alternatives (logprob.hip)
extern "C" size_t vila_logprobs_workspace_bytes(int n) { return logprob_workspace_bytes(n); }
extern "C" int vila_logprobs_slice_width(int vocab) { return vocab >= 1 ? logprob_slice_width(vocab) : 0; }
extern "C" int vila_logprobs_f32(const float* logits, int64_t ld, int n, int vocab, const int64_t* token, int top_n, const int32_t* rec, int rec_bias,
                                 const VilaLogprobOut* out, void* workspace, vila_stream_t stream) {
    static_assert(VILA_LOGPROBS_MAX_TOP == LP_TOP, "the header's record width is the kernel's");
    VILA_REQUIRE(out != nullptr, "logprobs: the output descriptor is NULL");
    VILA_REQUIRE((uintptr_t)workspace % 8 == 0, "logprobs: the workspace must be 8-byte aligned");
    return launch_logprobs(logits, ld, n, vocab, token, top_n, rec, rec_bias, out->token_logprob, out->top_logprob, out->top_id, out->max_rec, workspace, S(stream));
}
extern "C" size_t vila_sample_workspace_bytes(void) { return sample_workspace_bytes(); }
extern "C" int vila_sample_f32(const float* logits, int n, const VilaSampling* sp, const int32_t* counter, int64_t* out, void* workspace,
                               float* dist_out, vila_stream_t stream) {
    VILA_REQUIRE(sp != nullptr && logits != nullptr && out != nullptr && workspace != nullptr, "sample: NULL argument");
    return launch_sample(logits, n, sp->temperature, sp->top_k, sp->top_p, sp->seed, sp->seed_dev, counter, out, workspace, dist_out, S(stream));
}
// no decode step sets an error any more: always 0, kept so that existing bindings still link (vila_hip.h)
extern "C" int vila_llm_decode_chain_error(void*, vila_stream_t) { return 0; }

// The batch-1 step: ql == nullptr runs the bf16 projections, otherwise the int4 layers' W4A16 GEMVs (the lm_head stays bf16 either way, as
// AWQ / TinyChat keep it fp16).  Only the four projection launches of a layer differ between the two.
static int decode_step_impl(const VilaLlmWeights* w, const VilaLlmLayerW4* ql, const VilaKvCache* cache, const VilaDecodeState* st,
                            void* workspace, size_t workspace_bytes, const VilaSampling* sp, vila_stream_t stream, const VilaPenalties* pen,
                            const VilaConstraints* con) {
    const VilaLlmShape& sh = w->shape;
    hipStream_t s = S(stream);
    const bool w4 = ql != nullptr;
    const char* fn = w4 ? "llm_decode_w4" : "llm_decode";
    VILA_REQUIRE(cache != nullptr && st != nullptr, "%s: cache/state is NULL", fn);
    const bool scratch = pen != nullptr || con != nullptr;         // (the constrained step's workspace is the penalised step's)
    VILA_REQUIRE(workspace_bytes >= (scratch ? vila_llm_decode_penalized_workspace_bytes(&sh, cache->max_ctx) : vila_llm_decode_workspace_bytes(&sh, cache->max_ctx)),
                 "%s: workspace too small", fn);
    const int H = sh.hidden, F = sh.inter, hd = sh.head_dim, QS = sh.q_heads * hd, KS = sh.kv_heads * hd;
    const int ns = dec_splits(cache->max_ctx);
    Arena a(workspace, workspace_bytes);
    bf16_t* x = a.take<bf16_t>(H);
    bf16_t* x2 = a.take<bf16_t>(H);
    bf16_t* q = a.take<bf16_t>(QS);
    bf16_t* act = a.take<bf16_t>(F);
    float* part_o = a.take<float>((size_t)ns * QS);
    float* part_ml = a.take<float>((size_t)ns * sh.q_heads * 2);
    const int n_pick = gemv_grid_blocks(sh.vocab);               // one (max, index) pair per lm_head block
    float* tv = a.take<float>(n_pick);
    int* ti = a.take<int>(n_pick);
    float* rope_cs = a.take<float>(hd);
    bf16_t* ao = a.take<bf16_t>(QS);
    void* smp_ws = a.take<char>(sample_workspace_bytes());
    // the penalised step (behind the plain step's layout): the processed logits and the pairs of its greedy pick
    float* pen_y = scratch ? a.take<float>(sh.vocab) : nullptr;
    float* pen_v = scratch ? a.take<float>(PEN_SOLO_SLICES) : nullptr;
    int* pen_i = scratch ? a.take<int>(PEN_SOLO_SLICES) : nullptr;
    VILA_REQUIRE(a.ok(), "%s: workspace arena overflow", fn);
    const size_t per_layer = (size_t)cache->n_slots * sh.kv_heads * cache->max_ctx * hd;

    // per-head blocks over 256-key slices whose partials meet in the o_proj GEMV's prologue (§4.3; the W4 GEMV's merge holds up to 7 x 16 heads)
    const bool split256 = decode_attn_mode() >= 1 && cache->max_ctx <= DEC_SHORT_CTX && hd == 128 && (!w4 || QS <= 7 * 16 * 128);
    VILA_TRY(launch_decode_prologue(B(w->embed), st->token, x, H, sh.vocab, st->pos, rope_cs, hd, sh.rope_theta, s));
    bf16_t* cur = x; bf16_t* nxt = x2;
    for (int l = 0; l < sh.n_layers; ++l) {
        const VilaLlmLayer& L = w->layers[l];
        const VilaLlmLayerW4 Q = w4 ? ql[l] : VilaLlmLayerW4{};
        bf16_t* kc = B(cache->k) + l * per_layer; bf16_t* vc = B(cache->v) + l * per_layer;
        if (w4) {
            GemvW4Args qa{};
            qa.x = cur; qa.norm_w = B(L.ln1_w); qa.eps = sh.rms_eps; qa.Wq = (const uint32_t*)Q.qkv_q; qa.Wsz = (const uint32_t*)Q.qkv_sz;
            qa.bias = B(L.bq); qa.K = H; qa.N = QS + 2 * KS; qa.mode = 3; qa.q_out = q; qa.kcache = kc; qa.vcache = vc; qa.pos_ptr = st->pos;
            qa.rope_cs = rope_cs; qa.nq = sh.q_heads; qa.nkv = sh.kv_heads; qa.hd = hd; qa.max_ctx = cache->max_ctx;
            VILA_TRY(launch_gemv_w4(qa, s));
        } else {
            VILA_REQUIRE(qkv_fused(L.wq, L.wk, L.wv, L.bq, L.bk, L.bv, QS, KS, H), "llm_decode: q/k/v projection weights and biases must be views of one fused [q+2kv, hidden] buffer");
            QkvDecodeArgs qa{};
            qa.x = cur; qa.norm_w = B(L.ln1_w); qa.eps = sh.rms_eps; qa.Wqkv = B(L.wq); qa.bqkv = B(L.bq); qa.q_out = q;
            qa.kcache = kc; qa.vcache = vc; qa.pos_ptr = st->pos; qa.K = H; qa.nq = sh.q_heads; qa.nkv = sh.kv_heads; qa.hd = hd;
            qa.max_ctx = cache->max_ctx; qa.rope_cs = rope_cs;
            VILA_TRY(launch_qkv_decode(qa, s));
        }
        AttnDecodeArgs ad{};
        ad.q = q; ad.kcache = kc; ad.vcache = vc; ad.o = ao; ad.part_o = part_o; ad.part_ml = part_ml; ad.pos_ptr = st->pos;
        ad.nq = sh.q_heads; ad.nkv = sh.kv_heads; ad.hd = hd; ad.max_ctx = cache->max_ctx; ad.n_splits = ns; ad.scale = 1.0f / sqrtf((float)hd);
        ad.split256 = split256 ? 1 : 0;
        VILA_TRY(launch_attn_decode(ad, s));
        GemvArgs o{};
        o.x = ao; o.W = B(L.wo); o.residual = cur; o.y = nxt; o.N = H; o.K = QS; o.mode = 0;
        if (split256) { o.mode = 2; o.part_o = part_o; o.part_ml = part_ml; o.pos_ptr = st->pos; o.n_splits = cdiv(cache->max_ctx, 256); o.split_keys = 256; }
        VILA_TRY(proj_gemv(o, w4, Q.o_q, Q.o_sz, s));
        GemvArgs gu{};
        gu.x = nxt; gu.norm_w = B(L.ln2_w); gu.eps = sh.rms_eps; gu.W = B(L.w_gate); gu.W2 = B(L.w_up); gu.y = act; gu.N = F; gu.K = H; gu.mode = 1;
        VILA_TRY(proj_gemv(gu, w4, Q.gateup_q, Q.gateup_sz, s));
        GemvArgs dn{};
        dn.x = act; dn.W = B(L.w_down); dn.residual = nxt; dn.y = cur; dn.N = H; dn.K = F; dn.mode = 0;
        VILA_TRY(proj_gemv(dn, w4, Q.down_q, Q.down_sz, s));
    }
    // the head: final RMSNorm + lm_head rows -> fp32 logits (152 064 x 3584: 1.09 GB, 7 TB/s in gemv_kernel<0,7>).  The last layer's residual
    // stream is in `x`: o_proj writes x2 and down_proj writes x back, so every layer ends where it began.
    GemvArgs lm{};
    lm.x = x; lm.norm_w = B(w->norm_w); lm.eps = sh.rms_eps; lm.W = B(w->lm_head); lm.y_f32 = st->logits; lm.N = sh.vocab; lm.K = H; lm.mode = 0;
    // greedy: every lm_head block also reduces its rows to one (max, index) pair, and one small launch merges the pairs, writes the token and
    // advances the state; sampled: the sampler reads the logits, then the advance
    // penalised: lm_head without its fused pick, then one launch that bumps the count of the consumed token (st->token still holds it), writes the
    // processed row to pen_y and leaves its greedy pairs; the pick reads pen_y, st->logits stays raw
    // constrained: behind the penalties (in place on pen_y then), the automaton advances by the consumed token and masks the row (constrain.hip)
    if (sp == nullptr && !scratch) { lm.amax_v = tv; lm.amax_i = ti; }
    VILA_TRY(launch_gemv(lm, s));
    const float* pick_src = st->logits;
    if (pen != nullptr) {
        const Penalties P{pen->repetition, pen->presence, pen->frequency, pen->counts, pen->ld_counts};
        VILA_TRY(launch_penalize(st->logits, sh.vocab, 1, sh.vocab, P, st->token, pen_y, sh.vocab, PEN_SOLO_SLICES, sp != nullptr ? nullptr : pen_v,
                                 sp != nullptr ? nullptr : pen_i, s));
        pick_src = pen_y;
    }
    if (con != nullptr) {
        const Constraints Cn{con->state, con->cls, con->ld_cls, con->next, con->ld_next, con->n_classes};
        VILA_TRY(launch_constrain(pick_src, sh.vocab, 1, sh.vocab, Cn, st->token, pen_y, sh.vocab, PEN_SOLO_SLICES, sp != nullptr ? nullptr : pen_v,
                                  sp != nullptr ? nullptr : pen_i, s));
        pick_src = pen_y;
    }
    if (sp != nullptr) {
        VILA_TRY(launch_sample(pick_src, sh.vocab, sp->temperature, sp->top_k, sp->top_p, sp->seed, sp->seed_dev, st->pos, st->token, smp_ws, nullptr, s));
        VILA_TRY(launch_decode_advance(st->pos, st->token, st->out_ids, st->n_out, st->max_out, s));
    } else if (scratch) {
        VILA_TRY(launch_argmax_pick_advance(pen_v, pen_i, PEN_SOLO_SLICES, st->token, st->pos, st->out_ids, st->n_out, st->max_out, s));
    } else {
        VILA_TRY(launch_argmax_pick_advance(tv, ti, n_pick, st->token, st->pos, st->out_ids, st->n_out, st->max_out, s));
    }
    return 0;
}

// =================================================================================================
// Batched decode step (decode_batch.hip)
// =================================================================================================
// A sampled batched step keeps the greedy step's workspace layout and puts the sampler's candidates behind it: with `sp` set, the step's share of
// *workspace_bytes shrinks to the greedy size and `out` points at the tail.
struct BatchSamplingWs { const BatchSampling* sp; void* ws; };
static int batch_sampling_of(const VilaBatchSampling* sp, const VilaLlmShape* sh, int n, int max_ctx, void* workspace, size_t* workspace_bytes,
                             BatchSampling* bs, BatchSamplingWs* out, bool prefix = false) {
    out->sp = nullptr; out->ws = nullptr;
    if (sp == nullptr) return 0;
    VILA_REQUIRE(sp->temperature != nullptr && sp->top_k != nullptr && sp->top_p != nullptr && sp->seed != nullptr,
                 "llm_decode_batch_sample: a per-row parameter array is NULL");
    VILA_REQUIRE(n >= 1 && n <= 16, "llm_decode_batch_sample: 1..16 sequences (got %d)", n);
    VILA_REQUIRE(max_ctx >= 1 && max_ctx <= BDEC_MAX_CTX, "llm_decode_batch_sample: caches up to %d positions (got %d)", BDEC_MAX_CTX, max_ctx);
    const size_t head = align_up(prefix ? bdecode_prefix_workspace_bytes(sh->hidden, sh->inter, sh->q_heads * sh->head_dim, sh->head_dim, n, max_ctx)
                                        : bdecode_workspace_bytes(sh->hidden, sh->inter, sh->q_heads * sh->head_dim, sh->head_dim, n, max_ctx), 256);
    VILA_REQUIRE(!prefix || *workspace_bytes >= head + sample_batch_workspace_bytes(n),
                 "llm_decode_batch_prefix_sample: the step needs the workspace of vila_llm_decode_batch_prefix*_sample_workspace_bytes (%d positions)", max_ctx);
    VILA_REQUIRE(max_ctx <= BDEC_SHORT_CTX || *workspace_bytes >= head + sample_batch_workspace_bytes(n),
                 "llm_decode_batch_sample: caches beyond 2048 positions need the workspace of vila_llm_decode_batch*_sample_workspace_bytes_ctx (%d positions)",
                 max_ctx);
    VILA_REQUIRE(*workspace_bytes >= head + sample_batch_workspace_bytes(n), "llm_decode_batch_sample: workspace too small");
    *bs = BatchSampling{sp->temperature, sp->top_k, sp->top_p, sp->seed};
    out->sp = bs; out->ws = (char*)workspace + head;
    *workspace_bytes = head;
    return 0;
}
// the sizes by capacity: up to 2048 positions what the functions without `_ctx` return, beyond that room for the walking attention's partials.
// Two sizes, greedy and sampled: the W4 step lays its workspace out as the bf16 step does.
static size_t decode_batch_ws_ctx(const VilaLlmShape* s, int n, int max_ctx, bool sample) {
    const size_t b = bdecode_workspace_bytes(s->hidden, s->inter, s->q_heads * s->head_dim, s->head_dim, n, max_ctx);
    return sample ? align_up(b, 256) + sample_batch_workspace_bytes(n) : b;
}
extern "C" size_t vila_llm_decode_batch_workspace_bytes(const VilaLlmShape* s, int n) { return decode_batch_ws_ctx(s, n, BDEC_SHORT_CTX, false); }
extern "C" size_t vila_llm_decode_batch_sample_workspace_bytes(const VilaLlmShape* s, int n) { return decode_batch_ws_ctx(s, n, BDEC_SHORT_CTX, true); }
extern "C" size_t vila_llm_decode_batch_w4_workspace_bytes(const VilaLlmShape* s, int n) { return decode_batch_ws_ctx(s, n, BDEC_SHORT_CTX, false); }
extern "C" size_t vila_llm_decode_batch_w4_sample_workspace_bytes(const VilaLlmShape* s, int n) { return decode_batch_ws_ctx(s, n, BDEC_SHORT_CTX, true); }
extern "C" size_t vila_llm_decode_batch_workspace_bytes_ctx(const VilaLlmShape* s, int n, int max_ctx) { return decode_batch_ws_ctx(s, n, max_ctx, false); }
extern "C" size_t vila_llm_decode_batch_sample_workspace_bytes_ctx(const VilaLlmShape* s, int n, int max_ctx) { return decode_batch_ws_ctx(s, n, max_ctx, true); }
extern "C" size_t vila_llm_decode_batch_w4_workspace_bytes_ctx(const VilaLlmShape* s, int n, int max_ctx) { return decode_batch_ws_ctx(s, n, max_ctx, false); }
extern "C" size_t vila_llm_decode_batch_w4_sample_workspace_bytes_ctx(const VilaLlmShape* s, int n, int max_ctx) { return decode_batch_ws_ctx(s, n, max_ctx, true); }

// What the batched step and the verify step read of the model: the layer tables (ql stays empty without int4 layers) and the model arguments, with the
// fused q/k/v (bf16) or contiguous-bias and int4-buffer (W4) requirements per layer.  fn names the entry point in the messages.
struct BTables { std::vector<BLayer> layers; std::vector<BLayerW4> ql; BDecodeArgs m; };
static int blayer_tables(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const char* fn, BTables* t) {
    const bool w4 = qlayers != nullptr;
    const VilaLlmShape& sh = w->shape;
    const int QS = sh.q_heads * sh.head_dim, KS = sh.kv_heads * sh.head_dim;
    t->layers.resize(sh.n_layers);
    t->ql.resize(w4 ? sh.n_layers : 0);
    for (int l = 0; l < sh.n_layers; ++l) {
        const VilaLlmLayer& L = w->layers[l];
        if (w4) {
            const VilaLlmLayerW4& Q = qlayers[l];
            VILA_REQUIRE(L.bq != nullptr && B(L.bk) == B(L.bq) + QS && B(L.bv) == B(L.bk) + KS,
                         "%s: the q/k/v biases must be one contiguous q|k|v vector (layer %d)", fn, l);
            VILA_REQUIRE(Q.qkv_q && Q.qkv_sz && Q.o_q && Q.o_sz && Q.gateup_q && Q.gateup_sz && Q.down_q && Q.down_sz,
                         "%s: int4 layer %d has a NULL buffer", fn, l);
            t->layers[l] = BLayer{L.ln1_w, nullptr, L.bq, nullptr, L.ln2_w, nullptr, nullptr, nullptr};
            t->ql[l] = BLayerW4{Q.qkv_q, Q.qkv_sz, Q.o_q, Q.o_sz, Q.gateup_q, Q.gateup_sz, Q.down_q, Q.down_sz};
        } else {
            VILA_REQUIRE(qkv_fused(L.wq, L.wk, L.wv, L.bq, L.bk, L.bv, QS, KS, sh.hidden),
                         "%s: q/k/v projection weights and biases must be views of one fused [q+2kv, hidden] buffer", fn);
            t->layers[l] = BLayer{L.ln1_w, L.wq, L.bq, L.wo, L.ln2_w, L.w_gate, L.w_up, L.w_down};
        }
    }
    t->m = BDecodeArgs{w->embed, w->norm_w, w->lm_head, sh.hidden, sh.inter, sh.n_layers, sh.q_heads, sh.kv_heads, sh.head_dim, sh.vocab, sh.rms_eps, sh.rope_theta};
    return 0;
}
// The batched step: qlayers == nullptr runs the bf16 projections; otherwise the four projections of every layer are read from the int4 layers
// (gemv_w4_batch.hip) and embed, norms, the fused q|k|v biases and the bf16 lm_head come from `w`, whose projection pointers are not read (empty
// after quantize_w4(release_bf16=True)).  sp != nullptr: a per-row pick (sample.hip's batched sampler) instead of the greedy pair; everything
// before the pick is the same launches.
// px != nullptr: the step of a session with a shared prompt prefix (attn_decode.hip): cache->n_slots counts the prefix slot, and the workspace is the
// prefix step's, which a plain one never reaches.
static int decode_step_batch_impl(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const VilaKvCache* cache, const VilaDecodeBatch* st,
                                  void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp, vila_stream_t stream,
                                  const VilaDecodePrefix* px = nullptr, const Penalties* pen = nullptr, float* pen_out = nullptr,
                                  const Constraints* con = nullptr, bool any_k = false, const BLora* lora = nullptr) {
    const char* fn = qlayers != nullptr ? "llm_decode_batch_w4" : "llm_decode_batch";
    VILA_REQUIRE(w != nullptr && cache != nullptr && st != nullptr && workspace != nullptr, "%s: NULL argument", fn);
    BTables t{};
    VILA_TRY(blayer_tables(w, qlayers, fn, &t));
    BatchSampling bs{};
    BatchSamplingWs sw{};
    VILA_TRY(batch_sampling_of(sp, &w->shape, st->n, cache->max_ctx, workspace, &workspace_bytes, &bs, &sw, px != nullptr));
    const BPrefix bp = px != nullptr ? BPrefix{px->prefix_slot, px->shared_len, px->uses} : BPrefix{};
    return bdecode_step(t.m, t.layers.data(), B(cache->k), B(cache->v), cache->max_ctx, cache->n_slots, st->n, st->pos, st->token, st->out_ids, st->n_out,
                        st->max_out, st->logits, workspace, workspace_bytes, S(stream), qlayers != nullptr ? t.ql.data() : nullptr, sw.sp, sw.ws,
                        px != nullptr ? &bp : nullptr, pen, pen_out, con, any_k, lora);
}
// the four steps of a prefix session and their workspace sizes (two sizes, greedy and sampled, as above)
static size_t decode_batch_prefix_ws(const VilaLlmShape* s, int n, int max_ctx, bool sample) {
    const size_t b = bdecode_prefix_workspace_bytes(s->hidden, s->inter, s->q_heads * s->head_dim, s->head_dim, n, max_ctx);
    return sample ? align_up(b, 256) + sample_batch_workspace_bytes(n) : b;
}
extern "C" size_t vila_llm_decode_batch_prefix_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx) { return decode_batch_prefix_ws(s, n, max_ctx, false); }
extern "C" size_t vila_llm_decode_batch_prefix_sample_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx) { return decode_batch_prefix_ws(s, n, max_ctx, true); }
extern "C" size_t vila_llm_decode_batch_prefix_w4_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx) { return decode_batch_prefix_ws(s, n, max_ctx, false); }
extern "C" size_t vila_llm_decode_batch_prefix_w4_sample_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx) { return decode_batch_prefix_ws(s, n, max_ctx, true); }
extern "C" int vila_llm_decode_step_batch_prefix(const VilaLlmWeights* w, const VilaKvCache* cache, const VilaDecodeBatch* st, const VilaDecodePrefix* prefix,
                                                 void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    VILA_REQUIRE(prefix != nullptr, "llm_decode_batch_prefix: the prefix descriptor is NULL");
    return decode_step_batch_impl(w, nullptr, cache, st, workspace, workspace_bytes, nullptr, stream, prefix);
}
extern "C" int vila_llm_decode_step_batch_prefix_sample(const VilaLlmWeights* w, const VilaKvCache* cache, const VilaDecodeBatch* st,
                                                        const VilaDecodePrefix* prefix, void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp,
                                                        vila_stream_t stream) {
    VILA_REQUIRE(prefix != nullptr && sp != nullptr, "llm_decode_batch_prefix_sample: the prefix descriptor or the sampling parameters are NULL");
    return decode_step_batch_impl(w, nullptr, cache, st, workspace, workspace_bytes, sp, stream, prefix);
}
extern "C" int vila_llm_decode_step_batch_prefix_w4(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const VilaKvCache* cache, const VilaDecodeBatch* st,
                                                    const VilaDecodePrefix* prefix, void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    VILA_REQUIRE(prefix != nullptr && qlayers != nullptr, "llm_decode_batch_prefix_w4: NULL argument");
    return decode_step_batch_impl(w, qlayers, cache, st, workspace, workspace_bytes, nullptr, stream, prefix);
}
extern "C" int vila_llm_decode_step_batch_prefix_w4_sample(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const VilaKvCache* cache,
                                                           const VilaDecodeBatch* st, const VilaDecodePrefix* prefix, void* workspace, size_t workspace_bytes,
                                                           const VilaBatchSampling* sp, vila_stream_t stream) {
    VILA_REQUIRE(prefix != nullptr && qlayers != nullptr && sp != nullptr, "llm_decode_batch_prefix_w4_sample: NULL argument");
    return decode_step_batch_impl(w, qlayers, cache, st, workspace, workspace_bytes, sp, stream, prefix);
}
extern "C" int vila_llm_decode_step_batch(const VilaLlmWeights* w, const VilaKvCache* cache, const VilaDecodeBatch* st,
                                          void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    return decode_step_batch_impl(w, nullptr, cache, st, workspace, workspace_bytes, nullptr, stream);
}
extern "C" int vila_llm_decode_step_batch_sample(const VilaLlmWeights* w, const VilaKvCache* cache, const VilaDecodeBatch* st,
                                                 void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp, vila_stream_t stream) {
    VILA_REQUIRE(sp != nullptr, "llm_decode_batch_sample: sampling parameters are NULL");
    return decode_step_batch_impl(w, nullptr, cache, st, workspace, workspace_bytes, sp, stream);
}
extern "C" int vila_llm_decode_step_batch_w4(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const VilaKvCache* cache, const VilaDecodeBatch* st,
                                             void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    VILA_REQUIRE(qlayers != nullptr, "llm_decode_batch_w4: NULL argument");
    return decode_step_batch_impl(w, qlayers, cache, st, workspace, workspace_bytes, nullptr, stream);
}
extern "C" int vila_llm_decode_step_batch_w4_sample(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const VilaKvCache* cache, const VilaDecodeBatch* st,
                                                    void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp, vila_stream_t stream) {
    VILA_REQUIRE(sp != nullptr, "llm_decode_batch_w4_sample: sampling parameters are NULL");
    VILA_REQUIRE(qlayers != nullptr, "llm_decode_batch_w4: NULL argument");
    return decode_step_batch_impl(w, qlayers, cache, st, workspace, workspace_bytes, sp, stream);
}
// The penalised batched step (penalty.hip): qlayers, prefix and sp nullable — bf16 / W4, plain / shared prefix, greedy / sampled in one entry.  One
// workspace size for all of them: the sampled step's (plain or prefix), and behind it the processed rows [n][vocab].
static size_t decode_batch_penalized_head(const VilaLlmShape* s, int n, int max_ctx, bool prefix) {
    return align_up(prefix ? decode_batch_prefix_ws(s, n, max_ctx, true) : decode_batch_ws_ctx(s, n, max_ctx, true), 256);
}
extern "C" size_t vila_llm_decode_batch_penalized_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx, int prefix) {
    return decode_batch_penalized_head(s, n, max_ctx, prefix != 0) + align_up((size_t)(n > 0 ? n : 0) * s->vocab * 4, 256) + 256;
}
extern "C" int vila_llm_decode_step_batch_penalized(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const VilaKvCache* cache, const VilaDecodeBatch* st,
                                                    const VilaDecodePrefix* prefix, void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp,
                                                    const VilaPenalties* pen, vila_stream_t stream) {
    const char* fn = "llm_decode_batch_penalized";
    VILA_REQUIRE(w != nullptr && cache != nullptr && st != nullptr && workspace != nullptr, "%s: NULL argument", fn);
    VILA_TRY(penalties_ok(pen, w->shape.vocab, fn));
    VILA_REQUIRE(st->n >= 1 && st->n <= 16, "%s: 1..16 sequences (got %d)", fn, st->n);
    VILA_REQUIRE(cache->max_ctx >= 1 && cache->max_ctx <= BDEC_MAX_CTX, "%s: caches up to %d positions (got %d)", fn, BDEC_MAX_CTX, cache->max_ctx);
    VILA_REQUIRE(workspace_bytes >= vila_llm_decode_batch_penalized_workspace_bytes(&w->shape, st->n, cache->max_ctx, prefix != nullptr),
                 "%s: the step needs the workspace of vila_llm_decode_batch_penalized_workspace_bytes", fn);
    const size_t head = decode_batch_penalized_head(&w->shape, st->n, cache->max_ctx, prefix != nullptr);
    const Penalties P{pen->repetition, pen->presence, pen->frequency, pen->counts, pen->ld_counts};
    return decode_step_batch_impl(w, qlayers, cache, st, workspace, head, sp, stream, prefix, &P, (float*)((char*)workspace + head));
}
// The constrained batched step (constrain.hip): as the penalised one, with pen nullable too; its workspace is the penalised step's.
extern "C" size_t vila_llm_decode_batch_constrained_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx, int prefix) {
    return vila_llm_decode_batch_penalized_workspace_bytes(s, n, max_ctx, prefix);
}
extern "C" int vila_llm_decode_step_batch_constrained(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const VilaKvCache* cache, const VilaDecodeBatch* st,
                                                      const VilaDecodePrefix* prefix, void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp,
                                                      const VilaPenalties* pen, const VilaConstraints* con, vila_stream_t stream) {
    const char* fn = "llm_decode_batch_constrained";
    VILA_REQUIRE(w != nullptr && cache != nullptr && st != nullptr && workspace != nullptr, "%s: NULL argument", fn);
    if (pen != nullptr) VILA_TRY(penalties_ok(pen, w->shape.vocab, fn));
    VILA_TRY(constraints_ok(con, w->shape.vocab, fn));
    VILA_REQUIRE(st->n >= 1 && st->n <= 16, "%s: 1..16 sequences (got %d)", fn, st->n);
    VILA_REQUIRE(cache->max_ctx >= 1 && cache->max_ctx <= BDEC_MAX_CTX, "%s: caches up to %d positions (got %d)", fn, BDEC_MAX_CTX, cache->max_ctx);
    VILA_REQUIRE(workspace_bytes >= vila_llm_decode_batch_constrained_workspace_bytes(&w->shape, st->n, cache->max_ctx, prefix != nullptr),
                 "%s: the step needs the workspace of vila_llm_decode_batch_constrained_workspace_bytes", fn);
    const size_t head = decode_batch_penalized_head(&w->shape, st->n, cache->max_ctx, prefix != nullptr);
    const Penalties P = pen != nullptr ? Penalties{pen->repetition, pen->presence, pen->frequency, pen->counts, pen->ld_counts} : Penalties{};
    const Constraints Cn{con->state, con->cls, con->ld_cls, con->next, con->ld_next, con->n_classes};
    return decode_step_batch_impl(w, qlayers, cache, st, workspace, head, sp, stream, prefix, pen != nullptr ? &P : nullptr, (float*)((char*)workspace + head), &Cn);
}
// The sampled batched step that serves every top_k >= 0 (sample.hip, launch_sample_batch(any_k)): qlayers, prefix, pen and con nullable — bf16 / W4,
// plain / shared prefix, with or without penalties and automata in one entry; sp is required (the option is the sampled pick's).  One workspace size
// for all of them, the constrained step's: without pen and con the rows behind the head stay unused.  Everything in front of the pick is the launches
// of the step without the option, so st->logits holds the same bits.
extern "C" size_t vila_llm_decode_batch_any_k_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx, int prefix) {
    return vila_llm_decode_batch_penalized_workspace_bytes(s, n, max_ctx, prefix);
}
extern "C" int vila_llm_decode_step_batch_any_k(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const VilaKvCache* cache, const VilaDecodeBatch* st,
                                                const VilaDecodePrefix* prefix, void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp,
                                                const VilaPenalties* pen, const VilaConstraints* con, vila_stream_t stream) {
    const char* fn = "llm_decode_batch_any_k";
    VILA_REQUIRE(w != nullptr && cache != nullptr && st != nullptr && workspace != nullptr && sp != nullptr, "%s: NULL argument", fn);
    if (pen != nullptr) VILA_TRY(penalties_ok(pen, w->shape.vocab, fn));
    if (con != nullptr) VILA_TRY(constraints_ok(con, w->shape.vocab, fn));
    VILA_REQUIRE(st->n >= 1 && st->n <= 16, "%s: 1..16 sequences (got %d)", fn, st->n);
    VILA_REQUIRE(cache->max_ctx >= 1 && cache->max_ctx <= BDEC_MAX_CTX, "%s: caches up to %d positions (got %d)", fn, BDEC_MAX_CTX, cache->max_ctx);
    VILA_REQUIRE(workspace_bytes >= vila_llm_decode_batch_any_k_workspace_bytes(&w->shape, st->n, cache->max_ctx, prefix != nullptr),
                 "%s: the step needs the workspace of vila_llm_decode_batch_any_k_workspace_bytes", fn);
    const size_t head = decode_batch_penalized_head(&w->shape, st->n, cache->max_ctx, prefix != nullptr);
    const Penalties P = pen != nullptr ? Penalties{pen->repetition, pen->presence, pen->frequency, pen->counts, pen->ld_counts} : Penalties{};
    const Constraints Cn = con != nullptr ? Constraints{con->state, con->cls, con->ld_cls, con->next, con->ld_next, con->n_classes} : Constraints{};
    return decode_step_batch_impl(w, qlayers, cache, st, workspace, head, sp, stream, prefix, pen != nullptr ? &P : nullptr, (float*)((char*)workspace + head),
                                  con != nullptr ? &Cn : nullptr, true);
}
// The batched step with per-row LoRA adapters (lora_decode.hip): sp, pen and con nullable, any_k an option of sp — greedy / sampled, with or without
// penalties and automata in one entry.  One workspace size: the penalised step's (processed rows behind the head, unused without pen and con), and behind
// it the adapters' fp32 scratch T [n][3 r] and D [n][max(q + 2 kv, 2 inter)].  No int4 and no shared-prefix form.
static size_t decode_batch_lora_head(const VilaLlmShape* s, int n, int max_ctx) {
    return align_up(vila_llm_decode_batch_penalized_workspace_bytes(s, n, max_ctx, 0), 256);
}
extern "C" size_t vila_llm_decode_batch_lora_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx, int r) {
    const size_t rows = n > 0 ? n : 0, QKV = (size_t)(s->q_heads + 2 * s->kv_heads) * s->head_dim, wide = QKV > 2 * (size_t)s->inter ? QKV : 2 * (size_t)s->inter;
    return decode_batch_lora_head(s, n, max_ctx) + align_up(rows * 3 * (r > 0 ? r : 0) * 4, 256) + align_up(rows * wide * 4, 256);
}
extern "C" int vila_llm_decode_step_batch_lora(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const VilaKvCache* cache, const VilaDecodeBatch* st,
                                               const VilaDecodePrefix* prefix, const VilaLoraBank* bank, void* workspace, size_t workspace_bytes,
                                               const VilaBatchSampling* sp, const VilaPenalties* pen, const VilaConstraints* con, int any_k,
                                               vila_stream_t stream) {
    const char* fn = "llm_decode_batch_lora";
    VILA_REQUIRE(w != nullptr && cache != nullptr && st != nullptr && workspace != nullptr && bank != nullptr, "%s: NULL argument", fn);
    VILA_REQUIRE(qlayers == nullptr, "%s: the step with per-row adapters has no int4 form (the adapters add to bf16 projections)", fn);
    VILA_REQUIRE(prefix == nullptr, "%s: the step with per-row adapters has no shared-prefix form", fn);
    VILA_REQUIRE(!any_k || sp != nullptr, "%s: any top_k is an option of the sampled pick", fn);
    VILA_REQUIRE(bank->layers != nullptr && bank->scale != nullptr && bank->row_adapter != nullptr, "%s: the bank has a NULL pointer", fn);
    VILA_REQUIRE((bank->r == 16 || bank->r == 32 || bank->r == 48 || bank->r == 64) && bank->capacity >= 1 && bank->capacity <= LORA_MAX_SLOTS,
                 "%s: a bank of rank 16, 32, 48 or 64 with 1..%d slots (got r %d, %d slots)", fn, LORA_MAX_SLOTS, bank->r, bank->capacity);
    if (pen != nullptr) VILA_TRY(penalties_ok(pen, w->shape.vocab, fn));
    if (con != nullptr) VILA_TRY(constraints_ok(con, w->shape.vocab, fn));
    VILA_REQUIRE(st->n >= 1 && st->n <= 16, "%s: 1..16 sequences (got %d)", fn, st->n);
    VILA_REQUIRE(cache->max_ctx >= 1 && cache->max_ctx <= BDEC_MAX_CTX, "%s: caches up to %d positions (got %d)", fn, BDEC_MAX_CTX, cache->max_ctx);
    VILA_REQUIRE(workspace_bytes >= vila_llm_decode_batch_lora_workspace_bytes(&w->shape, st->n, cache->max_ctx, bank->r),
                 "%s: the step needs the workspace of vila_llm_decode_batch_lora_workspace_bytes", fn);
    const VilaLlmShape& sh = w->shape;
    std::vector<BLoraLayer> layers(sh.n_layers);
    for (int l = 0; l < sh.n_layers; ++l) {
        const VilaLoraBankLayer& L = bank->layers[l];
        VILA_REQUIRE(L.a_qkv && L.b_qkv && L.a_o && L.b_o && L.a_gateup && L.b_gateup && L.a_down && L.b_down, "%s: bank layer %d has a NULL buffer", fn, l);
        layers[l] = BLoraLayer{L.a_qkv, L.b_qkv, L.a_o, L.b_o, L.a_gateup, L.b_gateup, L.a_down, L.b_down};
    }
    const size_t head = decode_batch_penalized_head(&sh, st->n, cache->max_ctx, false), tail = decode_batch_lora_head(&sh, st->n, cache->max_ctx);
    float* T = (float*)((char*)workspace + tail);
    float* D = (float*)((char*)workspace + tail + align_up((size_t)st->n * 3 * bank->r * 4, 256));
    const BLora lora{layers.data(), bank->scale, bank->row_adapter, bank->capacity, bank->r, T, D};
    const Penalties P = pen != nullptr ? Penalties{pen->repetition, pen->presence, pen->frequency, pen->counts, pen->ld_counts} : Penalties{};
    const Constraints Cn = con != nullptr ? Constraints{con->state, con->cls, con->ld_cls, con->next, con->ld_next, con->n_classes} : Constraints{};
    return decode_step_batch_impl(w, nullptr, cache, st, workspace, head, sp, stream, nullptr, pen != nullptr ? &P : nullptr, (float*)((char*)workspace + head),
                                  con != nullptr ? &Cn : nullptr, any_k != 0, &lora);
}
// The verify step (speculative decoding, decode_batch.hip bverify_step): the layer tables are the batched step's, the state is one sequence's.
// sp != nullptr: the sampled form, whose four parameter arrays hold ONE entry each.
static int decode_step_verify_impl(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const VilaKvCache* cache, const VilaDecodeVerify* st,
                                   void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp, vila_stream_t stream, bool any_k = false,
                                   const BVerifyProc* proc = nullptr) {
    const char* fn = qlayers != nullptr ? "llm_decode_verify_w4" : "llm_decode_verify";
    VILA_REQUIRE(w != nullptr && cache != nullptr && st != nullptr && workspace != nullptr, "%s: NULL argument", fn);
    VILA_REQUIRE(sp == nullptr || (sp->temperature != nullptr && sp->top_k != nullptr && sp->top_p != nullptr && sp->seed != nullptr),
                 "%s_sample: a sampling parameter array is NULL", fn);
    const BatchSampling bs = sp != nullptr ? BatchSampling{sp->temperature, sp->top_k, sp->top_p, sp->seed} : BatchSampling{};
    BTables t{};
    VILA_TRY(blayer_tables(w, qlayers, fn, &t));
    BVerifyState v{st->n, st->slot, st->pos, st->token, st->n_draft, st->out_ids, st->n_out, st->max_out, st->logits, st->n_accept,
                   st->hist, st->n_hist, st->hist_cap, st->max_ngram, st->cand, st->n_cand};
    return bverify_step(t.m, t.layers.data(), B(cache->k), B(cache->v), cache->max_ctx, cache->n_slots, v, workspace, workspace_bytes, S(stream),
                        qlayers != nullptr ? t.ql.data() : nullptr, sp != nullptr ? &bs : nullptr, any_k, proc);
}
extern "C" size_t vila_llm_decode_verify_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx) {
    return bverify_workspace_bytes(s->hidden, s->inter, s->q_heads * s->head_dim, s->head_dim, n, max_ctx);
}
extern "C" size_t vila_llm_decode_verify_sample_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx) {
    return bverify_sample_workspace_bytes(s->hidden, s->inter, s->q_heads * s->head_dim, s->head_dim, n, max_ctx);
}
extern "C" int vila_llm_decode_step_verify_sample(const VilaLlmWeights* w, const VilaKvCache* cache, const VilaDecodeVerify* st, void* workspace,
                                                  size_t workspace_bytes, const VilaBatchSampling* sp, vila_stream_t stream) {
    VILA_REQUIRE(sp != nullptr, "llm_decode_verify_sample: sampling parameters are NULL");
    return decode_step_verify_impl(w, nullptr, cache, st, workspace, workspace_bytes, sp, stream);
}
extern "C" int vila_llm_decode_step_verify_w4_sample(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const VilaKvCache* cache,
                                                     const VilaDecodeVerify* st, void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp,
                                                     vila_stream_t stream) {
    VILA_REQUIRE(sp != nullptr, "llm_decode_verify_w4_sample: sampling parameters are NULL");
    VILA_REQUIRE(qlayers != nullptr, "llm_decode_verify_w4: NULL argument");
    return decode_step_verify_impl(w, qlayers, cache, st, workspace, workspace_bytes, sp, stream);
}
// the sampled verify step whose draws serve every top_k >= 0 (qlayers nullable: bf16 / W4 in one entry); the workspace is the sampled step's
extern "C" int vila_llm_decode_step_verify_any_k(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const VilaKvCache* cache, const VilaDecodeVerify* st,
                                                 void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp, vila_stream_t stream) {
    VILA_REQUIRE(sp != nullptr, "llm_decode_verify_any_k: sampling parameters are NULL");
    return decode_step_verify_impl(w, qlayers, cache, st, workspace, workspace_bytes, sp, stream, true);
}
// The processed verify step (decode_batch.hip bverify_step with a BVerifyProc): qlayers, sp, pen, con and lp nullable — bf16 / W4, greedy / sampled (any_k:
// every top_k >= 0), with penalties, an automaton and records in any mix, in one entry with one workspace size.  Everything is refused here, before a launch.
extern "C" size_t vila_llm_decode_verify_processed_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx) {
    return bverify_processed_workspace_bytes(s->hidden, s->inter, s->q_heads * s->head_dim, s->head_dim, n, max_ctx, s->vocab);
}
extern "C" int vila_llm_decode_step_verify_processed(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const VilaKvCache* cache, const VilaDecodeVerify* st,
                                                     void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp, int any_k, const VilaPenalties* pen,
                                                     const VilaConstraints* con, const VilaLogprobOut* lp, vila_stream_t stream) {
    const char* fn = "llm_decode_verify_processed";
    VILA_REQUIRE(w != nullptr && cache != nullptr && st != nullptr && workspace != nullptr, "%s: NULL argument", fn);
    VILA_REQUIRE(!any_k || sp != nullptr, "%s: any top_k is an option of the sampled step", fn);
    if (pen != nullptr) VILA_TRY(penalties_ok(pen, w->shape.vocab, fn));
    if (con != nullptr) VILA_TRY(constraints_ok(con, w->shape.vocab, fn));
    VILA_REQUIRE(lp == nullptr || (lp->token_logprob != nullptr && (lp->top_logprob == nullptr) == (lp->top_id == nullptr) && lp->max_rec >= 1),
                 "%s: the records need token_logprob, both top_logprob and top_id or neither, and max_rec >= 1", fn);
    VILA_REQUIRE(st->n >= 2 && st->n <= 16, "%s: 2..16 rows per step (got %d)", fn, st->n);
    VILA_REQUIRE(cache->max_ctx >= 1 && cache->max_ctx <= BDEC_MAX_CTX, "%s: caches up to %d positions (got %d)", fn, BDEC_MAX_CTX, cache->max_ctx);
    VILA_REQUIRE(workspace_bytes >= vila_llm_decode_verify_processed_workspace_bytes(&w->shape, st->n, cache->max_ctx),
                 "%s: the step needs the workspace of vila_llm_decode_verify_processed_workspace_bytes", fn);
    const Penalties P = pen != nullptr ? Penalties{pen->repetition, pen->presence, pen->frequency, pen->counts, pen->ld_counts} : Penalties{};
    const Constraints Cn = con != nullptr ? Constraints{con->state, con->cls, con->ld_cls, con->next, con->ld_next, con->n_classes} : Constraints{};
    const BVerifyProc pr{pen != nullptr ? &P : nullptr, con != nullptr ? &Cn : nullptr, lp != nullptr ? lp->token_logprob : nullptr,
                         lp != nullptr ? lp->top_logprob : nullptr, lp != nullptr ? lp->top_id : nullptr, lp != nullptr ? lp->max_rec : 0};
    return decode_step_verify_impl(w, qlayers, cache, st, workspace, workspace_bytes, sp, stream, any_k != 0, &pr);
}
// its launches on their own (operator level): the penalty and mask launches of n rows of ONE sequence, the commit behind an accept, one-sequence records
extern "C" int vila_logits_penalize_verify_f32(const float* logits, int64_t ld, int n, int vocab, const VilaPenalties* pen, const int64_t* token, float* out,
                                               int64_t ld_out, float* pick_v, int* pick_i, vila_stream_t stream) {
    VILA_REQUIRE(pen != nullptr, "logits_penalize_verify: the penalties are NULL");
    const Penalties P{pen->repetition, pen->presence, pen->frequency, pen->counts, pen->ld_counts};
    return launch_penalize_verify(logits, ld, n, vocab, P, token, out, ld_out, PEN_PICK_SLICES, pick_v, pick_i, S(stream));
}
extern "C" int vila_logits_constrain_verify_f32(const float* logits, int64_t ld, int n, int vocab, const VilaConstraints* con, const int64_t* token,
                                                int32_t* states_out, float* out, int64_t ld_out, float* pick_v, int* pick_i, vila_stream_t stream) {
    VILA_REQUIRE(logits != nullptr && out != nullptr && token != nullptr && states_out != nullptr, "logits_constrain_verify: NULL argument");
    VILA_REQUIRE(n >= 1 && n <= PEN_VERIFY_MAX_ROWS && vocab >= 1, "logits_constrain_verify: 1..%d rows of a non-empty vocabulary (got %d x %d)",
                 PEN_VERIFY_MAX_ROWS, n, vocab);
    VILA_TRY(constraints_ok(con, vocab, "logits_constrain_verify"));
    VILA_REQUIRE(ld >= vocab && ld_out >= vocab && (pick_v == nullptr) == (pick_i == nullptr), "logits_constrain_verify: a row stride below the vocabulary %d, or "
                 "one of the two pair arrays", vocab);
    const Constraints Cn{con->state, con->cls, con->ld_cls, con->next, con->ld_next, con->n_classes};
    VILA_TRY(launch_verify_chain(&Cn, token, n, vocab, states_out, nullptr, S(stream)));
    return launch_constrain_rows(logits, ld, n, vocab, Cn, states_out, out, ld_out, PEN_PICK_SLICES, pick_v, pick_i, S(stream));
}
extern "C" int vila_verify_commit(const VilaPenalties* pen, const VilaConstraints* con, int vocab, const int64_t* consumed, const int32_t* states,
                                  const int32_t* n_accept, int n, vila_stream_t stream) {
    VILA_REQUIRE(pen != nullptr || con != nullptr, "verify_commit: neither penalties nor an automaton");
    VILA_REQUIRE(vocab >= 1, "verify_commit: an empty vocabulary");
    if (pen != nullptr) VILA_TRY(penalties_ok(pen, vocab, "verify_commit"));
    if (con != nullptr) VILA_REQUIRE(con->state != nullptr, "verify_commit: the automaton's state is NULL");
    return launch_verify_commit(pen != nullptr ? pen->counts : nullptr, vocab, con != nullptr ? con->state : nullptr, consumed, states, n_accept, n, S(stream));
}
extern "C" int vila_logprobs_seq_f32(const float* logits, int64_t ld, int n, int vocab, const int64_t* token, int top_n, const int32_t* rec,
                                     const VilaLogprobOut* out, void* workspace, vila_stream_t stream) {
    VILA_REQUIRE(out != nullptr && rec != nullptr, "logprobs (one sequence): the output descriptor or the record indices are NULL");
    VILA_REQUIRE((uintptr_t)workspace % 8 == 0, "logprobs: the workspace must be 8-byte aligned");
    return launch_logprobs(logits, ld, n, vocab, token, top_n, rec, 0, out->token_logprob, out->top_logprob, out->top_id, out->max_rec, workspace, S(stream), true);
}
extern "C" int vila_llm_decode_step_verify(const VilaLlmWeights* w, const VilaKvCache* cache, const VilaDecodeVerify* st, void* workspace,
                                           size_t workspace_bytes, vila_stream_t stream) {
    return decode_step_verify_impl(w, nullptr, cache, st, workspace, workspace_bytes, nullptr, stream);
}
extern "C" int vila_llm_decode_step_verify_w4(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers, const VilaKvCache* cache, const VilaDecodeVerify* st,
                                              void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    VILA_REQUIRE(qlayers != nullptr, "llm_decode_verify_w4: NULL argument");
    return decode_step_verify_impl(w, qlayers, cache, st, workspace, workspace_bytes, nullptr, stream);
}
// the verify step's draft stage and its attention on their own (operator level)
extern "C" int vila_prompt_lookup_draft(const int64_t* hist, const int32_t* n_hist, int max_ngram, int n, int64_t* token, int32_t* n_draft,
                                        vila_stream_t stream) {
    VILA_REQUIRE(hist != nullptr && n_hist != nullptr, "prompt_lookup_draft: NULL argument");
    return launch_verify_draft(hist, n_hist, max_ngram, nullptr, nullptr, nullptr, n, token, n_draft, nullptr, nullptr, S(stream));
}
extern "C" size_t vila_attn_decode_verify_workspace_bytes(int n, int q_heads, int max_ctx) { return bverify_attn_workspace_bytes(n, q_heads, max_ctx); }
// the append prefill's attention on its own (attn.hip launch_attn_append)
extern "C" int vila_attn_append_bf16(const void* q, int64_t ldq, const void* kslot, const void* vslot, int past, int T, void* o, int64_t ldo, int q_heads,
                                     int kv_heads, int max_ctx, float scale, vila_stream_t stream) {
    VILA_REQUIRE(q != nullptr && kslot != nullptr && vslot != nullptr && o != nullptr, "attn_append: NULL pointer");
    return launch_attn_append(B(q), ldq, B(kslot), B(vslot), past, T, B(o), ldo, q_heads, kv_heads, max_ctx, scale, S(stream));
}
extern "C" int vila_attn_decode_verify_bf16(const void* q, int64_t ldq, const void* kslot, const void* vslot, const int32_t* pos, void* o, int64_t ldo, int n,
                                            int q_heads, int kv_heads, int max_ctx, float scale, void* workspace, size_t workspace_bytes,
                                            vila_stream_t stream) {
    return bverify_attn(B(q), ldq, B(kslot), B(vslot), pos, (bf16_t*)o, ldo, n, q_heads, kv_heads, max_ctx, scale, workspace, workspace_bytes, S(stream));
}
// the batched step's attention alone (operator level): the form is chosen as the step chooses it
extern "C" size_t vila_attn_decode_batch_workspace_bytes(int n_rows, int q_heads, int max_ctx) { return bdecode_attn_workspace_bytes(n_rows, q_heads, max_ctx); }
extern "C" int vila_attn_decode_batch_bf16(const void* q, int64_t ldq, const void* kcache, const void* vcache, int64_t slot_stride, const int32_t* pos, void* o,
                                           int64_t ldo, int n_rows, int q_heads, int kv_heads, int max_ctx, float scale, void* workspace,
                                           size_t workspace_bytes, vila_stream_t stream) {
    return bdecode_attn(B(q), ldq, B(kcache), B(vcache), slot_stride, pos, (bf16_t*)o, ldo, n_rows, q_heads, kv_heads, max_ctx, scale, workspace,
                        workspace_bytes, S(stream));
}
// the batch-1 step's attention on its own (operator level): AttnDecodeArgs filled the way decode_step_impl fills them, on a workspace that holds the
// step's partials ([splits of 64 keys][q_heads][128] + [..][2]).  `o_proj`: the 256-key slices, whose merge exists only in the o_proj GEMV's prologue
static_assert(VILA_ATTN_DECODE_HEAD == 0 && VILA_ATTN_DECODE_SLICES256 == 1 && VILA_ATTN_DECODE_SPLIT64 == 2, "attention forms of the batch-1 step");
extern "C" size_t vila_attn_decode_workspace_bytes(int q_heads, int max_ctx) {
    const size_t ns = dec_splits(max_ctx);
    return align_up(ns * q_heads * 128 * 4, 256) + align_up(ns * q_heads * 2 * 4, 256);
}
static int attn_decode_op(const void* q, const void* kslot, const void* vslot, const int32_t* pos, void* o, int q_heads, int kv_heads, int max_ctx, float scale,
                          int form, void* workspace, size_t workspace_bytes, float** part_o, float** part_ml, hipStream_t s) {
    VILA_REQUIRE(q && kslot && vslot && pos && workspace, "attn_decode: NULL argument");
    VILA_REQUIRE(q_heads >= 1 && kv_heads >= 1 && q_heads % kv_heads == 0 && q_heads / kv_heads <= DEC_MAXG,
                 "attn_decode: a GQA group of 1..%d query heads per kv head (got %d / %d heads)", DEC_MAXG, q_heads, kv_heads);
    VILA_REQUIRE((uintptr_t)q % 16 == 0 && (uintptr_t)kslot % 16 == 0 && (uintptr_t)vslot % 16 == 0 && (uintptr_t)workspace % 16 == 0,
                 "attn_decode: head_dim 128 rows, 16-byte aligned, a slot of [kv_heads][max_ctx][128]");
    if (form == VILA_ATTN_DECODE_SPLIT64)
        VILA_REQUIRE(max_ctx > DEC_SHORT_CTX && max_ctx <= BDEC_MAX_CTX, "attn_decode: the 64-key split serves caches of %d..%d positions (got %d)",
                     DEC_SHORT_CTX + 1, BDEC_MAX_CTX, max_ctx);
    else
        VILA_REQUIRE(max_ctx >= 1 && max_ctx <= DEC_SHORT_CTX, "attn_decode: the per-head forms serve caches of 1..%d positions (got %d)", DEC_SHORT_CTX, max_ctx);
    VILA_REQUIRE(workspace_bytes >= vila_attn_decode_workspace_bytes(q_heads, max_ctx), "attn_decode: workspace too small");
    const int ns = dec_splits(max_ctx);
    *part_o = (float*)workspace;
    *part_ml = (float*)((char*)workspace + align_up((size_t)ns * q_heads * 128 * 4, 256));
    AttnDecodeArgs ad{};
    ad.q = B(q); ad.kcache = B(kslot); ad.vcache = B(vslot); ad.o = (bf16_t*)o; ad.part_o = *part_o; ad.part_ml = *part_ml; ad.pos_ptr = pos;
    ad.nq = q_heads; ad.nkv = kv_heads; ad.hd = 128; ad.max_ctx = max_ctx; ad.n_splits = ns; ad.scale = scale;
    ad.split256 = form == VILA_ATTN_DECODE_SLICES256 ? 1 : 0;
    return launch_attn_decode(ad, s);
}
extern "C" int vila_attn_decode_bf16(const void* q, const void* kslot, const void* vslot, const int32_t* pos, void* o, int q_heads, int kv_heads, int max_ctx,
                                     float scale, int form, void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    VILA_REQUIRE(form == VILA_ATTN_DECODE_HEAD || form == VILA_ATTN_DECODE_SPLIT64,
                 "attn_decode: form %d has no attention output of its own (the 256-key slices meet in vila_attn_decode_oproj_bf16 / _w4)", form);
    VILA_REQUIRE(o != nullptr, "attn_decode: NULL argument");
    float *part_o, *part_ml;
    return attn_decode_op(q, kslot, vslot, pos, o, q_heads, kv_heads, max_ctx, scale, form, workspace, workspace_bytes, &part_o, &part_ml, S(stream));
}
static int attn_decode_oproj(const void* q, const void* kslot, const void* vslot, const int32_t* pos, const void* W, const void* Wq, const void* Wsz,
                             const void* residual, void* y, int N, int q_heads, int kv_heads, int max_ctx, float scale, void* workspace, size_t workspace_bytes,
                             vila_stream_t stream) {
    VILA_REQUIRE(y != nullptr && N >= 1 && (W != nullptr || (Wq != nullptr && Wsz != nullptr)), "attn_decode_oproj: NULL argument");
    const bool w4 = W == nullptr;
    VILA_REQUIRE(!w4 || q_heads <= 7 * 16, "attn_decode_oproj: the W4 merge holds up to %d heads (got %d)", 7 * 16, q_heads);
    hipStream_t s = S(stream);
    float *part_o, *part_ml;
    VILA_TRY(attn_decode_op(q, kslot, vslot, pos, nullptr, q_heads, kv_heads, max_ctx, scale, VILA_ATTN_DECODE_SLICES256, workspace, workspace_bytes, &part_o,
                            &part_ml, s));
    GemvArgs g{};
    g.x = B(workspace); g.W = B(W); g.residual = B(residual); g.y = B(y); g.N = N; g.K = q_heads * 128;       // x: never read in this mode
    g.mode = 2; g.part_o = part_o; g.part_ml = part_ml; g.pos_ptr = pos; g.n_splits = cdiv(max_ctx, 256); g.split_keys = 256;
    return proj_gemv(g, w4, Wq, Wsz, s);
}
extern "C" int vila_attn_decode_oproj_bf16(const void* q, const void* kslot, const void* vslot, const int32_t* pos, const void* W, const void* residual, void* y,
                                           int N, int q_heads, int kv_heads, int max_ctx, float scale, void* workspace, size_t workspace_bytes,
                                           vila_stream_t stream) {
    VILA_REQUIRE(W != nullptr, "attn_decode_oproj: NULL argument");
    return attn_decode_oproj(q, kslot, vslot, pos, W, nullptr, nullptr, residual, y, N, q_heads, kv_heads, max_ctx, scale, workspace, workspace_bytes, stream);
}
extern "C" int vila_attn_decode_oproj_w4(const void* q, const void* kslot, const void* vslot, const int32_t* pos, const void* Wq, const void* Wsz,
                                         const void* residual, void* y, int N, int q_heads, int kv_heads, int max_ctx, float scale, void* workspace,
                                         size_t workspace_bytes, vila_stream_t stream) {
    VILA_REQUIRE(Wq != nullptr && Wsz != nullptr, "attn_decode_oproj_w4: NULL argument");
    return attn_decode_oproj(q, kslot, vslot, pos, nullptr, Wq, Wsz, residual, y, N, q_heads, kv_heads, max_ctx, scale, workspace, workspace_bytes, stream);
}
// the prefix session's attention alone (operator level): shared_len_host = S where the host knows it, -1 where only the device does
extern "C" size_t vila_attn_decode_batch_prefix_workspace_bytes(int n_rows, int q_heads, int max_ctx) { return bprefix_attn_workspace_bytes(n_rows, q_heads, max_ctx); }
extern "C" int vila_attn_decode_batch_prefix_bf16(const void* q, int64_t ldq, const void* kcache, const void* vcache, int64_t slot_stride, int n_slots,
                                                  int prefix_slot, const int32_t* shared_len, int shared_len_host, const int32_t* uses, const int32_t* pos,
                                                  void* o, int64_t ldo, int n_rows, int q_heads, int kv_heads, int max_ctx, float scale, void* workspace,
                                                  size_t workspace_bytes, vila_stream_t stream) {
    return bprefix_attn(B(q), ldq, B(kcache), B(vcache), slot_stride, n_slots, prefix_slot, shared_len, shared_len_host, uses, pos, (bf16_t*)o, ldo, n_rows,
                        q_heads, kv_heads, max_ctx, scale, workspace, workspace_bytes, S(stream));
}
extern "C" void vila_decode_batch_force_slices(int nsl) { bdecode_force_slices(nsl); }
extern "C" int vila_decode_batch_slices(int max_ctx) { return bdecode_attn_slices(max_ctx); }

// the batched sampler on its own (operator level: no state advance)
extern "C" size_t vila_sample_batch_workspace_bytes(int n) { return sample_batch_workspace_bytes(n); }
extern "C" int vila_sample_batch_f32(const float* logits, int64_t ld_logits, int n, int vocab, const VilaBatchSampling* sp, const int32_t* counter, int64_t* out,
                                     void* workspace, float* dist_out, vila_stream_t stream) {
    VILA_REQUIRE(sp != nullptr && logits != nullptr && out != nullptr && workspace != nullptr, "sample_batch: NULL argument");
    const BatchSampling bs{sp->temperature, sp->top_k, sp->top_p, sp->seed};
    return launch_sample_batch(logits, ld_logits, n, vocab, bs, 1, counter, out, workspace, dist_out, nullptr, nullptr, nullptr, 0, S(stream));
}

// ... and with the rows of top_k = 0 or > 64 drawn by the exact path (four launches whatever n; the same workspace).  dense_out (nullable)
// [n][ld_dense]: such a row's distribution over the vocabulary; the other rows' entries are not written
extern "C" int vila_sample_batch_any_f32(const float* logits, int64_t ld_logits, int n, int vocab, const VilaBatchSampling* sp, const int32_t* counter, int64_t* out,
                                         void* workspace, float* dist_out, float* dense_out, int64_t ld_dense, vila_stream_t stream) {
    VILA_REQUIRE(sp != nullptr && logits != nullptr && out != nullptr && workspace != nullptr, "sample_batch_any: NULL argument");
    const BatchSampling bs{sp->temperature, sp->top_k, sp->top_p, sp->seed};
    return launch_sample_batch(logits, ld_logits, n, vocab, bs, 1, counter, out, workspace, dist_out, nullptr, nullptr, nullptr, 0, S(stream), true, dense_out, ld_dense);
}

// =================================================================================================
// hipGraph helpers
// =================================================================================================
extern "C" int vila_graph_begin(vila_stream_t stream) {
    VILA_HIP(hipStreamBeginCapture(S(stream), hipStreamCaptureModeThreadLocal));
    return 0;
}
extern "C" int vila_graph_end(vila_stream_t stream, void** graph_exec_out) {
    hipGraph_t g = nullptr;
    VILA_HIP(hipStreamEndCapture(S(stream), &g));
    hipGraphExec_t e = nullptr;
    hipError_t err = hipGraphInstantiate(&e, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (err != hipSuccess) VILA_FAIL(-2, "hipGraphInstantiate failed: %s", hipGetErrorString(err));
    *graph_exec_out = (void*)e;
    return 0;
}
extern "C" int vila_graph_launch(void* graph_exec, vila_stream_t stream) {
    VILA_HIP(hipGraphLaunch((hipGraphExec_t)graph_exec, S(stream)));
    return 0;
}
extern "C" int vila_graph_destroy(void* graph_exec) {
    if (graph_exec) VILA_HIP(hipGraphExecDestroy((hipGraphExec_t)graph_exec));
    return 0;
}

// =================================================================================================
// Operator-level exports
// =================================================================================================
extern "C" int vila_gemm_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, const void* W2, const void* bias,
                              const void* residual, int64_t ldr, void* C, int64_t ldc, int out_f32, int M, int N, int K, int epi,
                              vila_stream_t stream) {
    return gemm(B(A), lda, W, ldw, bias, B(residual), ldr, C, ldc, M, N, K, epi, S(stream), W2, out_f32);
}
extern "C" int vila_gemm_bf16_ws(const void* A, int64_t lda, const void* W, int64_t ldw, const void* W2, const void* bias,
                                 const void* residual, int64_t ldr, void* C, int64_t ldc, int out_f32, int M, int N, int K, int epi,
                                 void* ws, size_t ws_bytes, vila_stream_t stream) {
    return gemm(B(A), lda, W, ldw, bias, B(residual), ldr, C, ldc, M, N, K, epi, S(stream), W2, out_f32, (float*)ws, ws_bytes);
}
// C[M,N] = A . B^T (+bias)(+residual) with either operand stored contraction-major: dgrad (b_cm: B = W[K][N] as it lies) and wgrad
// (a_cm, b_cm: A = dY[K=tokens][M], B = X[K=tokens][N]) read the forward tensors in place, no transposed copies
extern "C" int vila_gemm_bf16_t(const void* A, int64_t lda, int a_cm, const void* W, int64_t ldw, int b_cm, const void* bias,
                                const void* residual, int64_t ldr, void* C, int64_t ldc, int M, int N, int K, void* ws, size_t ws_bytes,
                                vila_stream_t stream) {
    GemmArgs g;
    g.A = B(A); g.lda = lda; g.a_cm = a_cm ? 1 : 0; g.W = B(W); g.ldw = ldw; g.b_cm = b_cm ? 1 : 0; g.bias = B(bias);
    g.residual = B(residual); g.ldr = ldr; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.epi = EPI_NONE;
    g.ws = (float*)ws; g.ws_bytes = ws_bytes;
    return launch_gemm(g, S(stream));
}
extern "C" int vila_layernorm_bf16(const void* x, const void* w, const void* b, void* y, int rows, int cols, float eps, vila_stream_t stream) {
    return launch_layernorm(B(x), B(w), B(b), B(y), rows, cols, eps, S(stream));
}
extern "C" int vila_rmsnorm_bf16(const void* x, const void* w, void* y, int rows, int cols, float eps, vila_stream_t stream) {
    return launch_rmsnorm(B(x), B(w), B(y), rows, cols, eps, S(stream));
}
extern "C" int vila_space_to_depth_bf16(const void* x, void* y, int n_images, int grid, int channels, int k, vila_stream_t stream) {
    return launch_space_to_depth(B(x), B(y), n_images, grid, channels, k, S(stream));
}
extern "C" int vila_attn_fwd_bf16(const void* q, const void* k, const void* v, void* o, int64_t q_tok_stride, int64_t k_tok_stride,
                                  int64_t v_tok_stride, int64_t o_tok_stride, int q_head_stride, int k_head_stride, int v_head_stride,
                                  int o_head_stride, const int32_t* cu_seqlens, int n_seq, int total_tokens, int max_seqlen,
                                  int n_q_heads, int n_kv_heads, int head_dim, int causal, float scale, float* lse, vila_stream_t stream) {
    AttnArgs at{};
    at.q = B(q); at.k = B(k); at.v = B(v); at.o = B(o);
    at.q_tok_stride = q_tok_stride; at.k_tok_stride = k_tok_stride; at.v_tok_stride = v_tok_stride; at.o_tok_stride = o_tok_stride;
    at.q_head_stride = q_head_stride; at.k_head_stride = k_head_stride; at.v_head_stride = v_head_stride; at.o_head_stride = o_head_stride;
    at.cu_seqlens = cu_seqlens; at.n_seq = n_seq; at.total_tokens = total_tokens; at.max_seqlen = max_seqlen;
    at.n_q_heads = n_q_heads; at.n_kv_heads = n_kv_heads; at.head_dim = head_dim; at.causal = causal; at.scale = scale; at.lse = lse;
    return launch_attn_fwd(at, S(stream));
}
extern "C" int vila_gemv_bf16(const void* x, const void* norm_w, float eps, const void* W, const void* W2, const void* bias,
                              const void* residual, void* y_bf16, float* y_f32, int N, int K, int mode, vila_stream_t stream) {
    GemvArgs g{};
    g.x = B(x); g.norm_w = B(norm_w); g.eps = eps; g.W = B(W); g.W2 = B(W2); g.bias = B(bias); g.residual = B(residual);
    g.y = B(y_bf16); g.y_f32 = y_f32; g.N = N; g.K = K; g.mode = mode;
    return launch_gemv(g, S(stream));
}
extern "C" int vila_argmax_f32(const float* logits, int n, int64_t* out, void* workspace, vila_stream_t stream) {
    float* tv = (float*)workspace;
    int* ti = (int*)((char*)workspace + 2048);
    return launch_argmax(logits, n, out, tv, ti, S(stream));
}
extern "C" int vila_wave_sum_probe(const float* in, float* out_xor, float* out_shfl, int n_waves, vila_stream_t stream) {
    return launch_wave_sum_probe(in, out_xor, out_shfl, n_waves, S(stream));
}

// =================================================================================================
// Training operator exports (backward kernels + optimizer); orchestrated by vila_amd/train.py
// =================================================================================================
extern "C" int vila_transpose_bf16(const void* in, void* out, int R, int C, int64_t ldi, int64_t ldo, vila_stream_t stream) {
    return launch_transpose(B(in), B(out), R, C, ldi, ldo, S(stream));
}
extern "C" int vila_act_fwd_bf16(const void* z, void* y, int64_t n, int act, vila_stream_t stream) { return launch_act_fwd(B(z), B(y), n, act, S(stream)); }
extern "C" int vila_act_bwd_bf16(const void* z, const void* dy, void* dz, int64_t n, int act, vila_stream_t stream) {
    return launch_act_bwd(B(z), B(dy), B(dz), n, act, S(stream));
}
extern "C" int vila_silu_mul_fwd_bf16(const void* g, const void* u, void* a, int64_t n, vila_stream_t stream) {
    return launch_silu_mul_fwd(B(g), B(u), B(a), n, S(stream));
}
extern "C" int vila_silu_mul_bwd_bf16(const void* g, const void* u, const void* da, void* dg, void* du, int64_t n, vila_stream_t stream) {
    return launch_silu_mul_bwd(B(g), B(u), B(da), B(dg), B(du), n, S(stream));
}
extern "C" int vila_add_bf16(const void* a, const void* b, void* y, int64_t n, vila_stream_t stream) { return launch_add(B(a), B(b), B(y), n, S(stream)); }
extern "C" int vila_grad_accum_f32(float* acc, const void* g, void* out, int64_t n, int mode, vila_stream_t stream) {
    return launch_grad_accum(acc, B(g), B(out), n, mode, S(stream));
}
extern "C" int vila_colsum_bf16(const void* x, void* out, float* scratch, int R, int C, int64_t ld, int accumulate, int period, vila_stream_t stream) {
    return launch_colsum(B(x), B(out), scratch, R, C, ld, accumulate, period, S(stream));
}
extern "C" int vila_norm_bwd_bf16(const void* x, const void* w, const void* dy, void* dx, void* dw, void* db, float* scratch, int rows, int cols,
                                  float eps, int rms, int accumulate, vila_stream_t stream) {
    return launch_norm_bwd(B(x), B(w), B(dy), B(dx), B(dw), B(db), scratch, rows, cols, eps, rms, accumulate, S(stream));
}
extern "C" int vila_ce_loss_f32(const float* logits, const int64_t* labels, void* dlogits, float* loss, float* row_loss, int rows, int V, int64_t ldl, float scale,
                                vila_stream_t stream) {
    return launch_ce(logits, labels, B(dlogits), loss, row_loss, rows, V, ldl, scale, S(stream));
}
extern "C" int vila_scatter_add_rows_bf16(const void* src, void* dst, const int32_t* rows, int n, int H, vila_stream_t stream) {
    return launch_scatter_add_rows(B(src), B(dst), rows, n, H, S(stream));
}
extern "C" int vila_depth_to_space_bf16(const void* dy, void* dx, int n_images, int grid, int channels, int k, vila_stream_t stream) {
    return launch_depth_to_space(B(dy), B(dx), n_images, grid, channels, k, S(stream));
}
extern "C" int vila_im2col_bf16(const void* pixels, void* out, int n_images, int channels, int H, int W, int P, int Kp, vila_stream_t stream) {
    return launch_im2col(B(pixels), B(out), n_images, channels, H, W, P, Kp, S(stream));
}
extern "C" int vila_rope_table_f32(const int32_t* positions, float* cos_out, float* sin_out, int S_, int head_dim, float theta, vila_stream_t stream) {
    return launch_rope_table(positions, cos_out, sin_out, S_, head_dim, theta, S(stream));
}
extern "C" int vila_rope_fwd_bf16(void* qkv, const float* cs, const float* sn, const int32_t* positions, int S_, int nq, int nkv, int hd,
                                  vila_stream_t stream) {
    return launch_rope_kv(B(qkv), cs, sn, positions, nullptr, nullptr, nullptr, S_, nq, nkv, hd, 0, S(stream));
}
extern "C" int vila_rope_bwd_bf16(void* dqkv, const float* cs, const float* sn, int S_, int nq, int nkv, int hd, vila_stream_t stream) {
    return launch_rope_bwd(B(dqkv), cs, sn, S_, nq, nkv, hd, S(stream));
}
extern "C" int vila_attn_bwd_bf16_parts(const void* q, const void* k, const void* v, const void* o, const void* d_o, void* dq, void* dk, void* dv,
                                  const int64_t* tok_strides /*[8] q,k,v,o,do,dq,dk,dv*/, const int32_t* head_strides /*[8]*/,
                                  const int32_t* cu_seqlens, int n_seq, int total_tokens, int max_seqlen, int n_q_heads, int n_kv_heads,
                                  int head_dim, int causal, float scale, const float* lse, float* delta, int parts, vila_stream_t stream) {
    AttnBwdArgs a{};
    a.q = B(q); a.k = B(k); a.v = B(v); a.o = B(o); a.d_o = B(d_o); a.dq = B(dq); a.dk = B(dk); a.dv = B(dv);
    a.q_tok_stride = tok_strides[0]; a.k_tok_stride = tok_strides[1]; a.v_tok_stride = tok_strides[2]; a.o_tok_stride = tok_strides[3];
    a.do_tok_stride = tok_strides[4]; a.dq_tok_stride = tok_strides[5]; a.dk_tok_stride = tok_strides[6]; a.dv_tok_stride = tok_strides[7];
    a.q_head_stride = head_strides[0]; a.k_head_stride = head_strides[1]; a.v_head_stride = head_strides[2]; a.o_head_stride = head_strides[3];
    a.do_head_stride = head_strides[4]; a.dq_head_stride = head_strides[5]; a.dk_head_stride = head_strides[6]; a.dv_head_stride = head_strides[7];
    for (int i = 0; i < 8; ++i) VILA_REQUIRE(tok_strides[i] % 8 == 0 && head_strides[i] % 8 == 0, "attn_bwd: strides must be multiples of 8 elements");
    a.cu_seqlens = cu_seqlens; a.n_seq = n_seq; a.total_tokens = total_tokens; a.max_seqlen = max_seqlen;
    a.n_q_heads = n_q_heads; a.n_kv_heads = n_kv_heads; a.head_dim = head_dim; a.causal = causal; a.scale = scale; a.lse = lse; a.delta = delta;
    return launch_attn_bwd(a, S(stream), parts);
}
extern "C" int vila_attn_bwd_bf16(const void* q, const void* k, const void* v, const void* o, const void* d_o, void* dq, void* dk, void* dv,
                                  const int64_t* tok_strides, const int32_t* head_strides, const int32_t* cu_seqlens, int n_seq, int total_tokens,
                                  int max_seqlen, int n_q_heads, int n_kv_heads, int head_dim, int causal, float scale, const float* lse, float* delta,
                                  vila_stream_t stream) {
    return vila_attn_bwd_bf16_parts(q, k, v, o, d_o, dq, dk, dv, tok_strides, head_strides, cu_seqlens, n_seq, total_tokens, max_seqlen, n_q_heads,
                                    n_kv_heads, head_dim, causal, scale, lse, delta, 7, stream);
}
extern "C" int vila_adamw_step(float* master, float* m, float* v, const void* grad, void* param, int64_t n, float lr, float beta1, float beta2,
                               float eps, float weight_decay, int step, float grad_scale, vila_stream_t stream) {
    return launch_adamw(master, m, v, B(grad), B(param), n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, S(stream));
}
// same update, <= 32 VGPRs per lane: meant for a side stream, co-resident with the matrix kernels (see adamw_lean_kernel)
extern "C" int vila_adamw_step_lean(float* master, float* m, float* v, const void* grad, void* param, int64_t n, float lr, float beta1, float beta2,
                                    float eps, float weight_decay, int step, float grad_scale, vila_stream_t stream) {
    return launch_adamw_lean(master, m, v, B(grad), B(param), n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, S(stream));
}
extern "C" int vila_sumsq_bf16(const void* x, int64_t n, float* out, float* scratch, vila_stream_t stream) { return launch_sumsq(B(x), n, out, scratch, S(stream)); }
extern "C" size_t vila_colsum_scratch_floats(int rows, int cols) { return colsum_scratch_floats(rows, cols); }
extern "C" size_t vila_norm_bwd_scratch_floats(int rows, int cols) { return norm_bwd_scratch_floats(rows, cols); }

// dynamic_s2: merge_chessboard + area interpolation + concat + split_chessboard in one gather
extern "C" int vila_s2_merge_bf16(const void* feats, void* out, const int32_t* desc, int n_blocks, int grid, int channels, int n_scales,
                                  const int32_t* splits /*[host] n_scales-1*/, vila_stream_t stream) {
    int sp[4] = {1, 1, 1, 1};
    for (int k = 0; k < n_scales - 1 && k < 4; ++k) sp[k] = splits[k];
    return launch_s2_merge(B(feats), B(out), desc, n_blocks, grid, channels, n_scales, sp, S(stream));
}

extern "C" int vila_s2_merge_bwd_bf16(const void* dy, void* dx, const int32_t* tile_desc, int n_tiles, int grid, int channels, int n_scales,
                                      const int32_t* splits /*[host] n_scales-1*/, vila_stream_t stream) {
    int sp[4] = {1, 1, 1, 1};
    for (int k = 0; k < n_scales - 1 && k < 4; ++k) sp[k] = splits[k];
    return launch_s2_merge_bwd(B(dy), B(dx), tile_desc, n_tiles, grid, channels, n_scales, sp, S(stream));
}

// video encoders: BasicVideoEncoder (pool 1,1,1) / TSPVideoEncoder token assembly in one launch
extern "C" int vila_video_pool_bf16(const void* feats, void* out, int n_frames, int grid, int channels, int pool_t, int pool_h, int pool_w,
                                    const void* start_rows, int n_start, const void* end_rows, int n_end, vila_stream_t stream) {
    return launch_video_pool(B(feats), B(out), n_frames, grid, channels, pool_t, pool_h, pool_w, B(start_rows), n_start, B(end_rows), n_end, S(stream));
}
extern "C" int vila_video_pool_bwd_bf16(const void* dpooled, void* dfeats, int n_frames, int grid, int channels, int pool_t, int pool_h, int pool_w,
                                        int accumulate, vila_stream_t stream) {
    return launch_video_pool_bwd(B(dpooled), B(dfeats), n_frames, grid, channels, pool_t, pool_h, pool_w, accumulate, S(stream));
}

// =================================================================================================
// W4A16 operators: int4 group-128 weights of the decoder-layer projections, as decode GEMVs and prefill GEMMs
// =================================================================================================
extern "C" int vila_gemv_w4_bf16(const void* x, const void* norm_w, float eps, const void* Wq, const void* Wsz,
                                 const void* bias, const void* residual, void* y, int N, int K, int mode, vila_stream_t stream) {
    GemvW4Args g{};
    g.x = B(x); g.norm_w = B(norm_w); g.eps = eps; g.Wq = (const uint32_t*)Wq; g.Wsz = (const uint32_t*)Wsz;
    g.bias = B(bias); g.residual = B(residual); g.y = B(y); g.N = N; g.K = K; g.mode = mode;
    VILA_REQUIRE(mode == 0 || mode == 1, "vila_gemv_w4_bf16: mode must be 0 or 1");
    VILA_REQUIRE(x != nullptr && Wq != nullptr && Wsz != nullptr && y != nullptr, "vila_gemv_w4_bf16: NULL pointer");
    return launch_gemv_w4(g, S(stream));
}

extern "C" int vila_gemv_w4_batch_bf16(const void* x, int64_t ldx, int n, const void* Wq, const void* Wsz, const void* bias, const void* residual,
                                       void* y, int N, int K, int mode, vila_stream_t stream) {
    VILA_REQUIRE(mode == 0 || mode == 1, "vila_gemv_w4_batch_bf16: mode must be 0 or 1");
    VILA_REQUIRE(x != nullptr && Wq != nullptr && Wsz != nullptr && y != nullptr, "vila_gemv_w4_batch_bf16: NULL pointer");
    GemvW4BatchArgs g{};
    g.x = B(x); g.ldx = ldx; g.Wq = (const uint32_t*)Wq; g.Wsz = (const uint32_t*)Wsz; g.bias = B(bias); g.residual = B(residual); g.ldr = N;
    g.y = B(y); g.ldy = N; g.n = n; g.N = N; g.K = K; g.mode = mode;
    return launch_gemv_w4_batch(g, S(stream));
}

// ---- operator entries of the two fused q|k|v W4 kernels (include/vila_hip.h; tests/test_gpu_w4_elements.py) ------------------------------
// The decode steps' own launchers on caller-owned buffers: the argument structs filled as vila_llm_decode_step_w4 (mode 3) and the batched step
// (mode 2) fill them, launch_gemv_w4 / launch_gemv_w4_batch unchanged.  What the steps guarantee by construction is refused here first.
extern "C" int vila_qkv_w4_bf16(const void* x, const void* norm_w, float eps, const void* Wq, const void* Wsz, const void* bias, void* q_out,
                                void* kcache, void* vcache, const int32_t* pos, const float* rope_cs, int q_heads, int kv_heads, int head_dim,
                                int max_ctx, int K, vila_stream_t stream) {
    VILA_REQUIRE(x != nullptr && Wq != nullptr && Wsz != nullptr && q_out != nullptr && kcache != nullptr && vcache != nullptr && pos != nullptr &&
                 rope_cs != nullptr, "vila_qkv_w4_bf16: NULL pointer");
    VILA_REQUIRE(q_heads > 0 && kv_heads > 0 && head_dim > 0 && head_dim % 16 == 0 && max_ctx > 0 && K > 0,
                 "vila_qkv_w4_bf16: q_heads=%d, kv_heads=%d, head_dim=%d (a multiple of 16), max_ctx=%d, K=%d", q_heads, kv_heads, head_dim, max_ctx, K);
    GemvW4Args g{};
    g.x = B(x); g.norm_w = B(norm_w); g.eps = eps; g.Wq = (const uint32_t*)Wq; g.Wsz = (const uint32_t*)Wsz; g.bias = B(bias);
    g.K = K; g.N = (q_heads + 2 * kv_heads) * head_dim; g.mode = 3; g.q_out = B(q_out); g.kcache = B(kcache); g.vcache = B(vcache); g.pos_ptr = pos;
    g.rope_cs = rope_cs; g.nq = q_heads; g.nkv = kv_heads; g.hd = head_dim; g.max_ctx = max_ctx;
    return launch_gemv_w4(g, S(stream));
}
extern "C" int vila_qkv_w4_batch_bf16(const void* x, int64_t ldx, int n, const void* Wq, const void* Wsz, const void* bias, void* q_out, int64_t ldq,
                                      void* kcache, void* vcache, int64_t slot_stride, const int32_t* pos, const float* rope_cs, int q_heads, int kv_heads,
                                      int head_dim, int max_ctx, int K, vila_stream_t stream) {
    VILA_REQUIRE(x != nullptr && Wq != nullptr && Wsz != nullptr && q_out != nullptr && kcache != nullptr && vcache != nullptr && pos != nullptr &&
                 rope_cs != nullptr, "vila_qkv_w4_batch_bf16: NULL pointer");
    VILA_REQUIRE(q_heads > 0 && kv_heads > 0 && head_dim > 0 && max_ctx > 0 && K > 0 && ldx >= K && ldq >= (int64_t)q_heads * head_dim && slot_stride >= 0,
                 "vila_qkv_w4_batch_bf16: q_heads=%d, kv_heads=%d, head_dim=%d, max_ctx=%d, or a row stride shorter than its row", q_heads, kv_heads, head_dim, max_ctx);
    GemvW4BatchArgs g{};
    g.x = B(x); g.ldx = ldx; g.Wq = (const uint32_t*)Wq; g.Wsz = (const uint32_t*)Wsz; g.bias = B(bias);
    g.n = n; g.N = (q_heads + 2 * kv_heads) * head_dim; g.K = K; g.mode = 2;
    g.q_out = B(q_out); g.ldq = ldq; g.kcache = B(kcache); g.vcache = B(vcache); g.slot_stride = slot_stride;
    g.pos = pos; g.rope_cs = rope_cs; g.nq = q_heads; g.nkv = kv_heads; g.hd = head_dim; g.max_ctx = max_ctx;
    return launch_gemv_w4_batch(g, S(stream));
}
extern "C" size_t vila_gemm_w4_workspace_bytes(int M, int N, int K, int mode) { return gemm_w4_workspace_bytes(M, N, K, mode); }
extern "C" int vila_gemm_w4_bf16(const void* x, const void* Wq, const void* Wsz, const void* bias, const void* residual, void* y,
                                 int M, int N, int K, int mode, void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    VILA_REQUIRE(mode == 0 || mode == 1, "vila_gemm_w4_bf16: mode must be 0 or 1 (the q|k|v form is vila_gemm_w4_qkv_bf16)");
    GemmW4Args g{};
    g.x = B(x); g.Wq = (const uint32_t*)Wq; g.Wsz = (const uint32_t*)Wsz; g.bias = B(bias); g.residual = B(residual); g.y = B(y);
    g.M = M; g.N = N; g.K = K; g.mode = mode;
    return launch_gemm_w4(g, workspace, workspace_bytes, S(stream));
}
extern "C" int vila_gemm_w4_qkv_bf16(const void* x, const void* Wq, const void* Wsz, const void* bias, void* y, int M, int q_heads, int kv_heads,
                                     int head_dim, int K, void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    VILA_REQUIRE(q_heads > 0 && kv_heads > 0, "vila_gemm_w4_qkv_bf16: q_heads=%d, kv_heads=%d", q_heads, kv_heads);
    GemmW4Args g{};
    g.x = B(x); g.Wq = (const uint32_t*)Wq; g.Wsz = (const uint32_t*)Wsz; g.bias = B(bias); g.y = B(y);
    g.M = M; g.N = (q_heads + 2 * kv_heads) * head_dim; g.K = K; g.mode = 2; g.n_rope_heads = q_heads + kv_heads; g.hd = head_dim;
    return launch_gemm_w4(g, workspace, workspace_bytes, S(stream));
}

/* vila_hip.h — C ABI of libvila_hip.so: the MI355X (gfx950) implementation of NVILA's forward hot path.
 *
 * The reference (NVlabs/VILA) has no FFI/plugin API: its seams are Python module contracts.
 * Every entry point below names the reference interface it replaces.  Conventions:
 *   - every pointer is a DEVICE pointer in the caller's current HIP context unless marked [host];
 *   - the caller (PyTorch) owns weights, activations, KV cache and workspace; the library allocates nothing
 *     and keeps no device memory between calls;
 *   - all work is enqueued asynchronously on `stream`; nothing synchronises the device;
 *   - layouts are the reference's: nn.Linear.weight [out,in] row-major bf16, activations [tokens, channels] bf16,
 *     conv weight [out, C, P, P];
 *   - return 0 on success, <0 on error; vila_last_error() gives a thread-local message.  The Python shim turns a
 *     non-zero status into ValueError/RuntimeError with the reference's wording where one exists.
 *   - re-entrant per (device, stream); no thread-local HIP state is assumed (backward runs on autograd threads).
 */
#ifndef VILA_HIP_H
#define VILA_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vila_stream_t; /* hipStream_t */

const char* vila_last_error(void);
int vila_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * Vision tower — replaces SiglipVisionTower / VisionTower.forward + feature_select
 *   llava/model/multimodal_encoder/vision_encoder.py:44-52,133-177  (hidden_states[select_layer], "cls_patch")
 *   llava/model/multimodal_encoder/siglip/modeling_siglip.py:320-329 (embeddings), :728-764 (encoder layer),
 *   :389-439 (attention), :711-715 (MLP)
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
    int hidden, inter, heads, image, patch, channels;
    int n_layers_run;   /* layers actually executed = index of hidden_states[select_layer] (26 for so400m, -2) */
    float ln_eps;
} VilaVitShape;
typedef struct {
    const void *ln1_w, *ln1_b, *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo, *ln2_w, *ln2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} VilaVitLayer;
typedef struct {
    VilaVitShape shape;
    const void* patch_w;          /* [hidden, C, P, P] */
    const void* patch_b;          /* [hidden] */
    const void* pos_emb;          /* [ (image/patch)^2, hidden ] */
    const VilaVitLayer* layers;   /* [host] array of n_layers_run entries */
} VilaVitWeights;
size_t vila_vit_workspace_bytes(const VilaVitShape* s, int n_images);
/* pixels [B, C, image, image] bf16 NCHW  ->  out [B, (image/patch)^2, hidden] bf16 */
int vila_vit_forward(const VilaVitWeights* w, const void* pixels, int n_images, void* out,
                     void* workspace, size_t workspace_bytes, vila_stream_t stream);

/* W8A8 vision tower (BASELINE configs[4]; the reference's quantised numbers come from the external TinyChat
 * backend, README.md:87 — no code in-tree, so the format is defined here): the q/k/v (fused), out_proj, fc1 and fc2 linears of every
 * encoder layer run int8 x int8 -> int32 on the matrix cores with per-output-channel weight scales (w = wq * ws[n], symmetric,
 * ws[n] = max|W[n,:]| / 127) and per-token dynamic activation scales; everything else as vila_vit_forward (same call contract). */
typedef struct {
    const void *wqkv_q, *wo_q, *fc1_q, *fc2_q;        /* int8 [3*hidden][hidden], [hidden][hidden], [inter][hidden], [hidden][inter] */
    const float *wqkv_s, *wo_s, *fc1_s, *fc2_s;       /* fp32 per output row */
} VilaVitLayerW8;
size_t vila_vit_w8a8_workspace_bytes(const VilaVitShape* s, int n_images);
int vila_vit_forward_w8a8(const VilaVitWeights* w, const VilaVitLayerW8* qlayers /*[host]*/, const void* pixels, int n_images, void* out,
                          void* workspace, size_t workspace_bytes, vila_stream_t stream);
/* operator level: per-token dynamic int8 quantisation (scale[r] = max|x_r| / 127) and the W8A8 GEMM
 * C[M,N] = epi((Aq . Wq^T) * sx[m] * sw[n] + bias[n]) (+ residual), epi in {VILA_EPI_NONE, VILA_EPI_GELU_TANH}; K %% 16 == 0 */
int vila_quant_rows_i8(const void* x_bf16, void* q_i8, float* scale, int rows, int cols, vila_stream_t stream);
int vila_gemm_w8a8(const void* Aq, int64_t lda, const void* Wq, int64_t ldw, const float* sx, const float* sw, const void* bias,
                   const void* residual, int64_t ldr, void* C, int64_t ldc, int M, int N, int K, int epi, vila_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * mm_projector — replaces MultimodalProjector.forward (llava/model/multimodal_projector/base_projector.py:248-252)
 * for mlp_downsample (:145-153), mlp_downsample_2x2_fix (:155-162), mlp_downsample_3x3_fix (:163-174), including the
 * space-to-depth blocks flat_square / flat_square_2x2 / flat_square_3x3 (:58-71, :84-97, :110-123).
 * ------------------------------------------------------------------------------------------------------------ */
enum { VILA_PROJ_MLP_DOWNSAMPLE = 0, VILA_PROJ_MLP_DOWNSAMPLE_2X2_FIX = 1, VILA_PROJ_MLP_DOWNSAMPLE_3X3_FIX = 2 };
typedef struct {
    int kind;
    int in_dim;    /* vision hidden C */
    int out_dim;   /* LLM hidden */
    const void *ln1_w, *ln1_b;   /* layers.1 */
    const void *fc1_w, *fc1_b;   /* layers.2 */
    const void *ln2_w, *ln2_b;   /* layers.4 (3x3 only) */
    const void *fc2_w, *fc2_b;   /* layers.4 (2x2) / layers.5 (3x3) */
    const void *fc3_w, *fc3_b;   /* layers.7 (3x3 only) */
} VilaProjWeights;
size_t vila_proj_workspace_bytes(const VilaProjWeights* w, int n_images, int n_tokens);
int vila_proj_out_tokens(int kind, int n_tokens);
/* feat [B, N, C] bf16 (N a perfect square) -> out [B, N', out_dim] bf16 */
int vila_proj_forward(const VilaProjWeights* w, const void* feat, int n_images, int n_tokens, void* out,
                      void* workspace, size_t workspace_bytes, vila_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Embedding + splice — replaces llm.model.embed_tokens (llava_arch.py:429, encoders/image/basic.py:22-27) and the
 * per-token python splice loop of LlavaMetaForCausalLM._embed (llava_arch.py:457-479): dst[dst_row[i]] = src[src_row[i]].
 * The caller computes the row maps (integer work on the ids, no per-token host sync).
 * ------------------------------------------------------------------------------------------------------------ */
int vila_embed_tokens(const void* table, int64_t vocab, int hidden, const int64_t* ids, int n, void* out, vila_stream_t stream);
int vila_copy_rows(const void* src, void* dst, const int32_t* src_row /*nullable*/, const int32_t* dst_row /*nullable*/,
                   int n, int hidden, vila_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * LLM — replaces HF Qwen2ForCausalLM.forward / .generate as called from
 *   llava/model/language_model/llava_llama.py:134-141 (forward(inputs_embeds, attention_mask, position_ids, labels))
 *   llava/model/llava_arch.py:833 (llm.generate(inputs_embeds=..., attention_mask=...))
 * (third-party transformers==4.46.0, pyproject.toml:17; arithmetic per SURVEY.md Appendix B).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
    int hidden, inter, n_layers, q_heads, kv_heads, head_dim, vocab;
    float rms_eps, rope_theta;
} VilaLlmShape;
typedef struct {
    const void *ln1_w, *wq, *bq, *wk, *bk, *wv, *bv, *wo, *ln2_w, *w_gate, *w_up, *w_down;
} VilaLlmLayer;
typedef struct {
    VilaLlmShape shape;
    const void* embed;            /* [vocab, hidden] */
    const VilaLlmLayer* layers;   /* [host] */
    const void* norm_w;
    const void* lm_head;          /* [vocab, hidden] (== embed when tied) */
} VilaLlmWeights;
typedef struct {
    void* k;        /* [n_layers][n_slots][kv_heads][max_ctx][head_dim] bf16 */
    void* v;
    int max_ctx, n_slots;
} VilaKvCache;

size_t vila_llm_prefill_workspace_bytes(const VilaLlmShape* s, int total_tokens);
/* Prefill / teacher-forced forward over a packed token stream.
 *   embeds      [total_tokens, hidden] bf16 (spliced image+text embeddings)
 *   positions   [total_tokens] i32   (restart per sequence, llava_arch.py:751)
 *   cu_seqlens  [n_seq+1] i32 or NULL (one sequence)  — flash-attn varlen semantics of model/utils/packing.py:12-21
 *   seq_of_tok  [total_tokens] i32 or NULL: KV-cache slot per token
 *   cache       nullable: K/V are appended at `positions`
 *   last_rows   [n_last] i32 or NULL: rows whose logits are wanted -> last_logits [n_last, vocab] fp32
 *   all_logits  nullable [total_tokens, vocab] fp32 (training / parity)
 *   final_hidden nullable [total_tokens, hidden] bf16: output of model.norm
 *   layer_hidden nullable [(n_layers+1), total_tokens, hidden] bf16: residual stream taps (parity tests)
 */
int vila_llm_prefill(const VilaLlmWeights* w, const void* embeds, const int32_t* positions, const int32_t* cu_seqlens,
                     int n_seq, int total_tokens, int max_seqlen, const int32_t* seq_of_tok, const VilaKvCache* cache,
                     const int32_t* last_rows, int n_last, float* last_logits, float* all_logits, void* final_hidden,
                     void* layer_hidden, void* workspace, size_t workspace_bytes, vila_stream_t stream);

/* Greedy decode state for one sequence (slot 0 of the cache); everything lives on the device so a step can be
 * replayed from a hipGraph with no host round trip (replaces the python loop of GenerationMixin greedy search). */
typedef struct {
    int32_t* pos;        /* scalar: number of tokens already in the cache = position of the next token */
    int64_t* token;      /* scalar: token to feed (in) / token chosen by argmax (out) */
    int64_t* out_ids;    /* [max_out] generated ids, appended every step */
    int32_t* n_out;      /* scalar */
    int max_out;
    float* logits;       /* [vocab] fp32 logits of the last step (kept for parity tests) */
} VilaDecodeState;
size_t vila_llm_decode_workspace_bytes(const VilaLlmShape* s, int max_ctx);
/* number of kernel launches one decode step enqueues (what a captured hipGraph replays per token) */
int vila_llm_decode_launches(const VilaLlmShape* s, int max_ctx);
int vila_llm_decode_step(const VilaLlmWeights* w, const VilaKvCache* cache, const VilaDecodeState* st,
                         void* workspace, size_t workspace_bytes, vila_stream_t stream);
/* Always returns 0: no decode step reports a device-side error.  Kept, with its signature, so that existing bindings still link; it neither
 * reads the workspace nor touches the stream. */
int vila_llm_decode_chain_error(void* workspace, vila_stream_t stream);

/* generate(do_sample=True): what HF GenerationMixin.sample does after the forward — logits / temperature -> TopK -> TopP -> softmax ->
 * multinomial (server.py:101-102,185-187 sets temperature 0.2 / top_p 0.9; GenerationConfig's default top_k = 50 applies).  The whole
 * choice runs on the device (three short launches for top_k in 1..64; one exact radix-selection launch for any other k) so that a sampled step
 * replays from a hipGraph; the uniform number is splitmix64(seed, position of the token).  Parity with torch.multinomial is distributional,
 * not bitwise. */
typedef struct {
    float temperature;   /* > 0 */
    int top_k;           /* >= 0; 0 = no top-k filter (HF), k >= n = the same */
    float top_p;         /* (0, 1] */
    uint64_t seed;
    const uint64_t* seed_dev;   /* optional device scalar: when non-NULL the kernel reads the seed from it (a captured decode graph then
                                   serves every sampled request: the host updates 8 bytes instead of re-capturing) and `seed` is ignored */
} VilaSampling;
size_t vila_sample_workspace_bytes(void);
/* logits [n] fp32 -> *out; counter: device scalar mixed into the RNG (nullable); dist_out (nullable): the distribution actually sampled from —
 * top_k in 1..64: [64] probabilities followed by [64] int32 token ids (descending probability, -1 = unused slot); any other top_k: [n] dense
 * probabilities */
int vila_sample_f32(const float* logits, int n, const VilaSampling* sp, const int32_t* counter, int64_t* out, void* workspace,
                    float* dist_out, vila_stream_t stream);
int vila_llm_decode_step_sample(const VilaLlmWeights* w, const VilaKvCache* cache, const VilaDecodeState* st,
                                void* workspace, size_t workspace_bytes, const VilaSampling* sp, vila_stream_t stream);

/* Batched greedy decode step (serving: llava_arch.py:823-833 called with a batch, server.py:171-290 serving concurrent requests): ONE pass
 * over the weights advances n <= 16 sequences.  Row i lives in KV-cache slot i (cache->n_slots >= n, filled by vila_llm_prefill with
 * seq_of_tok = slot), consumes token[i] at position pos[i] and leaves its next token in token[i] / out_ids[i][n_out[i]++], pos[i]++.
 * Rows that hit EOS keep stepping (the host ignores what they produce).  head_dim 128.  Caches up to 2048 positions run with the workspace of
 * vila_llm_decode_batch_workspace_bytes; caches up to 32768 positions (Qwen2.5's max_position_embeddings) with the workspace of
 * vila_llm_decode_batch_workspace_bytes_ctx(shape, n, cache->max_ctx), which returns the same size up to 2048 positions.  Beyond 2048 the attention's
 * blocks walk several 256-key chunks of a row (GQA groups of 1, 2, 4, 7 or 8 query heads); a long cache with the short workspace is refused
 * before anything is enqueued.  The same holds for the _sample, _w4 and _w4_sample steps and their _ctx sizes. */
typedef struct {
    int n;               /* sequences */
    int32_t* pos;        /* [n] */
    int64_t* token;      /* [n] */
    int64_t* out_ids;    /* [n][max_out] */
    int32_t* n_out;      /* [n] */
    int max_out;
    float* logits;       /* [n][vocab] fp32 logits of the last step */
} VilaDecodeBatch;
size_t vila_llm_decode_batch_workspace_bytes(const VilaLlmShape* s, int n);
size_t vila_llm_decode_batch_workspace_bytes_ctx(const VilaLlmShape* s, int n, int max_ctx);
int vila_llm_decode_step_batch(const VilaLlmWeights* w, const VilaKvCache* cache, const VilaDecodeBatch* st,
                               void* workspace, size_t workspace_bytes, vila_stream_t stream);

/* Per-row sampling for the batched step: the choice of VilaSampling (top_k in 1..64), made for every row at once.  All four members are DEVICE
 * arrays of n entries that the kernels read at run time, so ONE captured hipGraph of the step serves any mix of rows: the host rewrites a row's
 * entries when a request joins or leaves.  A row whose temperature is <= 0 is a greedy row (largest logit, ties to the lower index, as the greedy
 * batched step picks).  A sampled row's token is bit for bit what vila_sample_f32 returns for the same logits row, parameters, seed and counter.
 * Values out of range are clamped on the device (top_k to 1..64, top_p to (0, 1]); checking them is the host's business. */
typedef struct {
    const float* temperature;   /* [n]; <= 0: greedy row */
    const int32_t* top_k;       /* [n]; 1..64 */
    const float* top_p;         /* [n]; (0, 1] */
    const uint64_t* seed;       /* [n] */
} VilaBatchSampling;
size_t vila_sample_batch_workspace_bytes(int n);
/* logits [n][vocab] fp32, rows ld_logits floats apart, n <= 16 -> out[n]; counter: device [n] mixed into each row's RNG (nullable = 0);
 * dist_out (nullable) [n][128]: per row 64 probabilities followed by 64 int32 token ids (descending probability, -1 = unused slot; a greedy
 * row: probability 1 on its token).  Three launches whatever n.  No state is advanced. */
int vila_sample_batch_f32(const float* logits, int64_t ld_logits, int n, int vocab, const VilaBatchSampling* sp, const int32_t* counter,
                          int64_t* out, void* workspace, float* dist_out, vila_stream_t stream);
/* vila_llm_decode_step_batch with that pick in place of the greedy one: row i draws with counter pos[i] (the position of the token it consumes,
 * read before it advances), then token / out_ids / n_out / pos move as in the greedy step.  The launches before the pick are the greedy step's,
 * so the logits are the same bits. */
size_t vila_llm_decode_batch_sample_workspace_bytes(const VilaLlmShape* s, int n);
size_t vila_llm_decode_batch_sample_workspace_bytes_ctx(const VilaLlmShape* s, int n, int max_ctx);
int vila_llm_decode_step_batch_sample(const VilaLlmWeights* w, const VilaKvCache* cache, const VilaDecodeBatch* st,
                                      void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp, vila_stream_t stream);

/* The batched step's attention on its own (operator level): row i of q [n_rows][ldq] (q_heads x 128 bf16) attends keys 0 .. pos[i] of cache slot i;
 * kcache / vcache are ONE layer's [slots][kv_heads][max_ctx][128] with slots `slot_stride` elements apart; o [n_rows][ldo] bf16.  max_ctx up to
 * 32768, GQA groups of 1, 2, 4, 7 or 8; the kernel form (one slice per 256-key chunk up to 2048 positions, walking blocks beyond) is chosen as
 * the step chooses it.  Two launches. */
size_t vila_attn_decode_batch_workspace_bytes(int n_rows, int q_heads, int max_ctx);
int vila_attn_decode_batch_bf16(const void* q, int64_t ldq, const void* kcache, const void* vcache, int64_t slot_stride, const int32_t* pos,
                                void* o, int64_t ldo, int n_rows, int q_heads, int kv_heads, int max_ctx, float scale,
                                void* workspace, size_t workspace_bytes, vila_stream_t stream);

/* Batched decode over a shared prompt prefix: several rows of a batch (ten questions about one video, n samples of one prompt) begin with the same
 * S positions, and the step reads their K/V once for all rows.  The cache has one slot more than the batch has rows, the PREFIX SLOT; its keys
 * 0 .. S - 1 are the common start.  S (`shared_len`, a device scalar, a multiple of 256 — the kernels round it down to one inside the slot) and the
 * per-row flags `uses` are read on the device, so one captured hipGraph serves any S and any mix of rows.
 *   uses[i] != 0  row i attends keys 0 .. S - 1 of the prefix slot and keys S .. pos[i] of its own slot i (pos[i] >= S is the host's duty).  Positions
 *                 stay absolute: RoPE uses pos[i] and the step's K/V lands at position pos[i] of slot i, as in the plain step.  Rows 0 .. S - 1 of
 *                 slot i are never read.
 *   uses[i] == 0  an ordinary row: keys 0 .. pos[i] of slot i, with the bits of vila_attn_decode_batch_bf16 in its walking form at the same slice count.
 * S = 0 or all flags 0 is an ordinary session.  Rows of the prefix slot at or beyond S are never read by a step (the host may stage a prefill there).
 * A sharing row's output does not depend on n, its row index or the other rows.  GQA groups of 1, 2, 4, 7 or 8, n <= 16, caches up to 32768. */
typedef struct {
    int prefix_slot;            /* slot of the cache that holds the prefix: n <= prefix_slot < cache->n_slots */
    const int32_t* shared_len;  /* device scalar S */
    const int32_t* uses;        /* device [n] */
} VilaDecodePrefix;
/* The attention alone (operator level): vila_attn_decode_batch_bf16's arguments, plus the cache's slot count, the prefix slot, the two device arrays
 * and shared_len_host = S where the host knows it (refused unless a multiple of 256 within max_ctx) or -1.  Three launches; the private phase is always
 * the walking form, and both slice counts follow vila_decode_batch_force_slices. */
size_t vila_attn_decode_batch_prefix_workspace_bytes(int n_rows, int q_heads, int max_ctx);
int vila_attn_decode_batch_prefix_bf16(const void* q, int64_t ldq, const void* kcache, const void* vcache, int64_t slot_stride, int n_slots,
                                       int prefix_slot, const int32_t* shared_len, int shared_len_host, const int32_t* uses, const int32_t* pos,
                                       void* o, int64_t ldo, int n_rows, int q_heads, int kv_heads, int max_ctx, float scale,
                                       void* workspace, size_t workspace_bytes, vila_stream_t stream);
/* The batched steps on such a session: vila_llm_decode_step_batch{,_sample} with the descriptor.  cache->n_slots counts the prefix slot
 * (1 <= n <= min(16, n_slots - 1)); the workspace is the prefix step's, and a plain step's workspace is refused before anything is enqueued.
 * The W4 pair is declared with the W4 steps below. */
size_t vila_llm_decode_batch_prefix_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx);
size_t vila_llm_decode_batch_prefix_sample_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx);
int vila_llm_decode_step_batch_prefix(const VilaLlmWeights* w, const VilaKvCache* cache, const VilaDecodeBatch* st, const VilaDecodePrefix* prefix,
                                      void* workspace, size_t workspace_bytes, vila_stream_t stream);
int vila_llm_decode_step_batch_prefix_sample(const VilaLlmWeights* w, const VilaKvCache* cache, const VilaDecodeBatch* st,
                                             const VilaDecodePrefix* prefix, void* workspace, size_t workspace_bytes,
                                             const VilaBatchSampling* sp, vila_stream_t stream);

/* Greedy speculative decoding with lookup drafts (HF generate(prompt_lookup_num_tokens=k)): one step runs n = k + 1 consecutive positions of ONE
 * sequence in ONE cache slot and keeps as many tokens as the model itself would have chosen one by one.  Three stages, all on the device, so one
 * hipGraph replay is one speculative step:
 *   draft    token[1..n_draft] = a guess at what follows token[0]: HF PromptLookupCandidateGenerator on hist[0 : n_hist] (ngram sizes
 *            min(max_ngram, n_hist - 1) .. 1, the earliest window equal to the last ngram ids that has a continuation, up to n - 1 ids of it), or in
 *            candidate mode (cand != NULL and *n_cand >= 0) cand[*n_out + j], j < n - 1, cut at *n_cand: the candidate is a prediction of out_ids,
 *            aligned by output index;
 *   forward  row i consumes token[i] at position pos + i of the slot (K/V appended there; rows at or past max_ctx append nothing) and attends keys
 *            0 .. min(pos + i, max_ctx - 1); the slot's K/V is read once for all rows (vila_attn_decode_verify_bf16).  Rows past 1 + n_draft are
 *            padding: what they append is overwritten by the next step before anything reads it;
 *   accept   a[i] = first index of the maximum of logits row i; m = the largest value <= n_draft with a[j] == token[j + 1] for all j < m; a[0..m] are
 *            appended to out_ids and hist (each up to its capacity), n_out, pos and n_hist move by m + 1 (n_hist stops at hist_cap),
 *            token[0] = a[m], n_accept = m.
 * A row's logits do not depend on the other rows or on n, so the ids are exactly those of a session that drafts nothing.  head_dim 128,
 * q_heads * head_dim == hidden, a GQA group of 1, 2, 4, 7 or 8, max_ctx <= 32768; anything else is refused before a launch.  n is 2..16. */
typedef struct {
    int n;               /* rows per step: 1 committed token + up to n - 1 drafts */
    int slot;            /* KV-cache slot the sequence lives in */
    int32_t* pos;        /* scalar: tokens in the cache = position of token[0] */
    int64_t* token;      /* [n]: token[0] in / out; token[1..] the drafts of the last step */
    int32_t* n_draft;    /* scalar (out): drafts the last step offered, 0 .. n - 1 */
    int64_t* out_ids;    /* [max_out] */
    int32_t* n_out;      /* scalar */
    int max_out;
    float* logits;       /* [n][vocab] fp32 logits of the last step */
    int32_t* n_accept;   /* scalar (out): drafts the last step accepted */
    int64_t* hist;       /* [hist_cap]: the prompt's ids followed by everything generated, token[0] last (NULL with a candidate: no history kept) */
    int32_t* n_hist;     /* scalar */
    int hist_cap;
    int max_ngram;       /* >= 1; HF's max_matching_ngram_size (default 2) */
    const int64_t* cand; /* nullable: a predicted output */
    const int32_t* n_cand; /* scalar; < 0: lookup mode although cand is set */
} VilaDecodeVerify;
size_t vila_llm_decode_verify_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx);
int vila_llm_decode_step_verify(const VilaLlmWeights* w, const VilaKvCache* cache, const VilaDecodeVerify* st,
                                void* workspace, size_t workspace_bytes, vila_stream_t stream);
/* The verify step for a SAMPLED request.  Draft and forward are the greedy step's launches (the logits are the same bits); only a[i] changes:
 *   draw     a[i] = the token vila_sample_f32 returns for logits row i with the request's temperature / top_k / top_p / seed and the counter
 *            pos + i — the position of the token row i consumes, which is the counter the solo sampled step uses at that position.  The draw is
 *            the batched sampler's (vila_sample_batch_f32), bit for bit.
 *   accept   the rule above with these a[i]: a draft is kept exactly when the draw hits it.
 * The draw behind a position is a pure function of (logits bits, parameters, seed, counter), and a row's logits do not depend on the step it runs
 * in, so the ids are exactly those of the same sampled session drafting nothing.  (HF's assisted sampling accepts a point-mass draft x with
 * probability p(x); "the draw hits x" has that same probability, coupled to the request's fixed random stream.)
 * `sp` describes ONE sequence: its four members are device arrays of ONE entry, and every row reads entry 0.  The host rewrites the four scalars
 * per request; the captured graph stays.  temperature <= 0 makes every row a greedy row (largest logit, ties to the lower index: the greedy
 * step's a[i]).  On the device top_k is clamped to 1..64 and top_p to (0, 1]; checking them is the host's business.
 * Workspace: vila_llm_decode_verify_sample_workspace_bytes (the greedy step's plus the sampler's candidates and the n draws). */
size_t vila_llm_decode_verify_sample_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx);
int vila_llm_decode_step_verify_sample(const VilaLlmWeights* w, const VilaKvCache* cache, const VilaDecodeVerify* st,
                                       void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp, vila_stream_t stream);
/* The draft stage on its own (lookup mode): hist [*n_hist] -> token[1 .. *n_draft], the rest of token[1 .. n - 1] = token[0]. */
int vila_prompt_lookup_draft(const int64_t* hist, const int32_t* n_hist, int max_ngram, int n, int64_t* token, int32_t* n_draft,
                             vila_stream_t stream);
/* The verify step's attention on its own: row i of q [n][ldq] (q_heads x 128 bf16) attends keys 0 .. min(*pos + i, max_ctx - 1) of ONE slot of one
 * layer, kslot / vslot [kv_heads][max_ctx][128]; o [n][ldo] bf16; n in 1..16.  Two launches; the slice count follows vila_decode_batch_force_slices. */
size_t vila_attn_decode_verify_workspace_bytes(int n, int q_heads, int max_ctx);
int vila_attn_decode_verify_bf16(const void* q, int64_t ldq, const void* kslot, const void* vslot, const int32_t* pos, void* o, int64_t ldo,
                                 int n, int q_heads, int kv_heads, int max_ctx, float scale, void* workspace, size_t workspace_bytes,
                                 vila_stream_t stream);

/* Causal attention with a key prefix, the append prefill's attention on its own: row i of q [T][ldq] (q_heads x 128 bf16) sits at position past + i
 * and attends keys 0 .. past + i of ONE slot of one layer, kslot / vslot [kv_heads][max_ctx][128], whose rows past .. past + T - 1 hold the K / V of
 * these same tokens; o [T][ldo] bf16.  past >= 0, T >= 1, past + T <= max_ctx <= 32768, q_heads % kv_heads == 0.  Rows of the slot at or beyond
 * past + T are never read.  One launch; the block form follows vila_attn_force_append (vila_hip_tuning.h). */
int vila_attn_append_bf16(const void* q, int64_t ldq, const void* kslot, const void* vslot, int past, int T, void* o, int64_t ldo,
                          int q_heads, int kv_heads, int max_ctx, float scale, vila_stream_t stream);

/* The batch-1 step's attention on its own (operator level): q [q_heads][128] bf16 attends keys 0 .. *pos of ONE slot of one layer, kslot / vslot
 * [kv_heads][max_ctx][128]; GQA groups of 1..8.  *pos must be below max_ctx: these kernels read *pos + 1 keys unguarded (the step's drivers refuse a
 * full cache before any launch).  The three forms of vila_llm_decode_step, launched as the step launches them:
 *   HEAD       one block per query head over the whole context, o [q_heads][128] bf16; max_ctx <= 2048;
 *   SLICES256  per-head blocks over 256-key slices whose partials are merged in the prologue of the o_proj GEMV (the step's default up to 2048
 *              positions).  The attention output exists only inside that GEMV, so the form is served by vila_attn_decode_oproj_bf16 / _w4:
 *              y[N] = W[N][q_heads * 128] . o (+ residual[N]), with W bf16 or int4 groups of 128 (the layout of vila_gemv_w4_bf16; q_heads <= 112);
 *   SPLIT64    64-key split-KV partials and a merge launch, o [q_heads][128] bf16; 2048 < max_ctx <= 32768. */
enum { VILA_ATTN_DECODE_HEAD = 0, VILA_ATTN_DECODE_SLICES256 = 1, VILA_ATTN_DECODE_SPLIT64 = 2 };
size_t vila_attn_decode_workspace_bytes(int q_heads, int max_ctx);
int vila_attn_decode_bf16(const void* q, const void* kslot, const void* vslot, const int32_t* pos, void* o, int q_heads, int kv_heads, int max_ctx,
                          float scale, int form, void* workspace, size_t workspace_bytes, vila_stream_t stream);
int vila_attn_decode_oproj_bf16(const void* q, const void* kslot, const void* vslot, const int32_t* pos, const void* W, const void* residual, void* y,
                                int N, int q_heads, int kv_heads, int max_ctx, float scale, void* workspace, size_t workspace_bytes,
                                vila_stream_t stream);
int vila_attn_decode_oproj_w4(const void* q, const void* kslot, const void* vslot, const int32_t* pos, const void* Wq, const void* Wsz,
                              const void* residual, void* y, int N, int q_heads, int kv_heads, int max_ctx, float scale, void* workspace,
                              size_t workspace_bytes, vila_stream_t stream);

/* hipGraph helpers: capture whatever is enqueued on `stream` between begin/end, replay it later. */
int vila_graph_begin(vila_stream_t stream);
int vila_graph_end(vila_stream_t stream, void** graph_exec_out);
int vila_graph_launch(void* graph_exec, vila_stream_t stream);
int vila_graph_destroy(void* graph_exec);

/* ------------------------------------------------------------------------------------------------------------
 * Operator-level entry points (used by the parity tests and by autograd wrappers)
 * ------------------------------------------------------------------------------------------------------------ */
enum { VILA_EPI_NONE = 0, VILA_EPI_GELU_TANH = 1, VILA_EPI_GELU_ERF = 2, VILA_EPI_GATEUP = 3 };
/* C[M,N] = epi(A[M,K] W[N,K]^T + bias[N]) + residual[M,N];  EPI_GATEUP: C = silu(A W^T) * (A W2^T) */
int vila_gemm_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, const void* W2, const void* bias,
                   const void* residual, int64_t ldr, void* C, int64_t ldc, int out_f32, int M, int N, int K, int epi,
                   vila_stream_t stream);
/* same, with an fp32 workspace (>= splits*M*N*4 bytes): lets under-filled grids (small M x N, long K) run split-K */
int vila_gemm_bf16_ws(const void* A, int64_t lda, const void* W, int64_t ldw, const void* W2, const void* bias,
                      const void* residual, int64_t ldr, void* C, int64_t ldc, int out_f32, int M, int N, int K, int epi,
                      void* ws, size_t ws_bytes, vila_stream_t stream);
/* Backward GEMMs on the forward tensors AS THEY LIE (replaces the transposed operand copies autograd's mm backward / cuBLAS NT-TN
 * variants stand for): C[M,N] = A.B^T (+bias)(+residual), bf16 out.  a_cm / b_cm = 1: that operand is stored contraction-major,
 * X[K][rows] with rows contiguous (lda / ldw = its stored leading dimension), instead of [rows][K]:
 *   dgrad  dX[T,K] = dY[T,N] . W[N,K]     : A = dY (a_cm 0), B = W   (b_cm 1, ldw = K),  contraction N
 *   wgrad  dW[N,K] = dY[T,N]^T . X[T,K]   : A = dY (a_cm 1, lda = N), B = X (b_cm 1, ldw = K), contraction T (any T; zero-filled tail)
 * A contraction-major operand needs rows %% 8 == 0.  ws (nullable): fp32 workspace enabling split-K on under-filled grids. */
int vila_gemm_bf16_t(const void* A, int64_t lda, int a_cm, const void* W, int64_t ldw, int b_cm, const void* bias,
                     const void* residual, int64_t ldr, void* C, int64_t ldc, int M, int N, int K, void* ws, size_t ws_bytes,
                     vila_stream_t stream);
/* (process-global tuning / test switches of the kernels live in include/vila_hip_tuning.h: they are NOT part of the drop-in boundary) */
int vila_layernorm_bf16(const void* x, const void* w, const void* b, void* y, int rows, int cols, float eps, vila_stream_t stream);
int vila_rmsnorm_bf16(const void* x, const void* w, void* y, int rows, int cols, float eps, vila_stream_t stream);
int vila_space_to_depth_bf16(const void* x, void* y, int n_images, int grid, int channels, int k, vila_stream_t stream);
/* q,k,v,o: [tokens][heads][head_dim] views given by element strides; cu_seqlens NULL => n_seq sequences of max_seqlen */
int vila_attn_fwd_bf16(const void* q, const void* k, const void* v, void* o, int64_t q_tok_stride, int64_t k_tok_stride,
                       int64_t v_tok_stride, int64_t o_tok_stride, int q_head_stride, int k_head_stride, int v_head_stride,
                       int o_head_stride, const int32_t* cu_seqlens, int n_seq, int total_tokens, int max_seqlen,
                       int n_q_heads, int n_kv_heads, int head_dim, int causal, float scale, float* lse, vila_stream_t stream);
int vila_gemv_bf16(const void* x, const void* norm_w, float eps, const void* W, const void* W2, const void* bias,
                   const void* residual, void* y_bf16, float* y_f32, int N, int K, int mode, vila_stream_t stream);
int vila_argmax_f32(const float* logits, int n, int64_t* out, void* workspace /* >= 4 KiB */, vila_stream_t stream);
/* Probe of the decode GEMVs' wave reduction: one wave per 64 inputs; lane l of wave w writes to out_xor[64 w + l] the sum the LDS-free xor
 * butterfly (row swaps + DPP) gives it and to out_shfl[64 w + l] the sum of the shuffle butterfly it replaces.  The two must agree bit for bit. */
int vila_wave_sum_probe(const float* in, float* out_xor, float* out_shfl, int n_waves, vila_stream_t stream);


/* ------------------------------------------------------------------------------------------------------------
 * SFT step: backward and optimizer operators.  They replace what autograd + cuBLAS +
 * flash_attn backward + torch.optim.AdamW do under HF Trainer.training_step (llava/train/transformer_normalize_monkey_patch.py:183-249).
 * dgrad / wgrad are vila_gemm_bf16 on transposed operands (vila_transpose_bf16).
 * ------------------------------------------------------------------------------------------------------------ */
int vila_transpose_bf16(const void* in, void* out, int rows, int cols, int64_t ld_in, int64_t ld_out, vila_stream_t stream);
int vila_act_fwd_bf16(const void* z, void* y, int64_t n, int act /*1 tanh-GELU, 2 erf-GELU*/, vila_stream_t stream);
int vila_act_bwd_bf16(const void* z, const void* dy, void* dz, int64_t n, int act, vila_stream_t stream);
int vila_silu_mul_fwd_bf16(const void* gate, const void* up, void* act, int64_t n, vila_stream_t stream);
int vila_silu_mul_bwd_bf16(const void* gate, const void* up, const void* dact, void* dgate, void* dup, int64_t n, vila_stream_t stream);
int vila_add_bf16(const void* a, const void* b, void* y, int64_t n, vila_stream_t stream);
/* Gradient accumulation across the micro-batches of one update (`--gradient_accumulation_steps`; HF Trainer adds each micro-batch's
 * backward into the fp32 / param-dtype .grad, transformer_normalize_monkey_patch.py:236-249): the running sum `acc` is fp32.
 * mode 0: acc = g;  mode 1: acc += g;  mode 2: out = bf16(acc + g) (acc untouched, out may alias g).  g, out: bf16[n]; n % 8 == 0. */
int vila_grad_accum_f32(float* acc, const void* g, void* out, int64_t n, int mode, vila_stream_t stream);
/* Reductions of the SFT step are DETERMINISTIC (round 6): every block writes fp32 partials into the caller's scratch and a second kernel adds
 * them in a fixed order — no atomics, so two identical steps produce identical bits (a resumed run equals the uninterrupted one). */
size_t vila_colsum_scratch_floats(int rows, int cols);
size_t vila_norm_bwd_scratch_floats(int rows, int cols);
#define VILA_SUMSQ_SCRATCH_FLOATS 2048
/* out[c] (+)= sum_r x[r][c] (scratch: vila_colsum_scratch_floats fp32); period > 0: out[p][c] = sum over rows r == p (mod period) (position-embedding gradient, no scratch) */
int vila_colsum_bf16(const void* x, void* out, float* scratch, int rows, int cols, int64_t ld, int accumulate, int period, vila_stream_t stream);
/* LayerNorm (rms=0) / RMSNorm (rms=1) backward; scratch = vila_norm_bwd_scratch_floats(rows, cols) fp32 */
int vila_norm_bwd_bf16(const void* x, const void* w, const void* dy, void* dx, void* dw, void* db, float* scratch, int rows, int cols,
                       float eps, int rms, int accumulate, vila_stream_t stream);
/* softmax-CE over fp32 logits rows: loss += sum_i (lse_i - z_i[label_i]) * scale ; dlogits = (softmax - onehot) * scale (bf16);
 * row_loss = scratch of `rows` floats (the per-row losses, summed in a fixed order) */
int vila_ce_loss_f32(const float* logits, const int64_t* labels, void* dlogits, float* loss, float* row_loss, int rows, int vocab, int64_t ld_logits,
                     float scale, vila_stream_t stream);
/* dst[rows[i]] += src[i] (embedding gradient); repeated ids are summed in fp32 in ascending i by the first occurrence's block and rounded once */
int vila_scatter_add_rows_bf16(const void* src, void* dst, const int32_t* rows, int n, int hidden, vila_stream_t stream);
int vila_depth_to_space_bf16(const void* dy, void* dx, int n_images, int grid, int channels, int k, vila_stream_t stream);
int vila_im2col_bf16(const void* pixels, void* out, int n_images, int channels, int H, int W, int patch, int k_padded, vila_stream_t stream);
int vila_rope_table_f32(const int32_t* positions, float* cos_out, float* sin_out, int n_tokens, int head_dim, float theta, vila_stream_t stream);
int vila_rope_fwd_bf16(void* qkv, const float* cos_t, const float* sin_t, const int32_t* positions, int n_tokens, int q_heads, int kv_heads,
                       int head_dim, vila_stream_t stream);
int vila_rope_bwd_bf16(void* dqkv, const float* cos_t, const float* sin_t, int n_tokens, int q_heads, int kv_heads, int head_dim, vila_stream_t stream);
/* flash-attention backward; tok_strides / head_strides: [8] host arrays for q,k,v,o,do,dq,dk,dv (elements) */
int vila_attn_bwd_bf16(const void* q, const void* k, const void* v, const void* o, const void* d_o, void* dq, void* dk, void* dv,
                       const int64_t* tok_strides, const int32_t* head_strides, const int32_t* cu_seqlens, int n_seq, int total_tokens,
                       int max_seqlen, int n_q_heads, int n_kv_heads, int head_dim, int causal, float scale, const float* lse, float* delta,
                       vila_stream_t stream);
/* the same in separately launchable parts (bit mask): 1 = delta = rowsum(dO o O) (needed by the other two), 2 = dQ, 4 = dK / dV.  The parts
 * share no output: once delta is done a caller may run dQ and dK / dV on different streams */
int vila_attn_bwd_bf16_parts(const void* q, const void* k, const void* v, const void* o, const void* d_o, void* dq, void* dk, void* dv,
                             const int64_t* tok_strides, const int32_t* head_strides, const int32_t* cu_seqlens, int n_seq, int total_tokens,
                             int max_seqlen, int n_q_heads, int n_kv_heads, int head_dim, int causal, float scale, const float* lse, float* delta,
                             int parts, vila_stream_t stream);
/* torch.optim.AdamW semantics on flat buffers: fp32 master/m/v, bf16 grad in (times grad_scale), bf16 param out */
int vila_adamw_step(float* master, float* m, float* v, const void* grad, void* param, int64_t n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int step, float grad_scale, vila_stream_t stream);
/* the same update from a kernel that allocates <= 32 VGPRs per lane, so that it can be co-resident with a 256x256 GEMM block on a side
 * stream (per-bucket optimizer overlapped with the backward of the layers below); results identical to vila_adamw_step */
int vila_adamw_step_lean(float* master, float* m, float* v, const void* grad, void* param, int64_t n, float lr, float beta1, float beta2,
                         float eps, float weight_decay, int step, float grad_scale, vila_stream_t stream);
/* *out += sum x^2 (global gradient norm); scratch = VILA_SUMSQ_SCRATCH_FLOATS floats */
int vila_sumsq_bf16(const void* x, int64_t n, float* out, float* scratch, vila_stream_t stream);


/* ------------------------------------------------------------------------------------------------------------
 * LoRA fine-tuning (reference llava/train/train.py:149-171, 648-706): the three skinny products of a rank-r adapter.  All operands bf16,
 * fp32 accumulation, `scale` applied to the fp32 accumulator before anything else is added, one rounding to bf16.  R, the skinny width,
 * is a multiple of 16 from 16 to 192 (q|k|v stacked at r = 64).  Every leading dimension is a multiple of 8 elements and every base
 * pointer 16-byte aligned; a call that breaks this returns -1 and launches nothing.  Same bits on every run: split sums are combined in
 * a fixed order from fp32 partials in `workspace` (vila_lora_*_workspace_bytes; nothing outside it is written), never with atomics.
 * ------------------------------------------------------------------------------------------------------------ */
size_t vila_lora_down_workspace_bytes(int M, int K, int R);
size_t vila_lora_up_workspace_bytes(int M, int N, int R);
size_t vila_lora_wgrad_workspace_bytes(int M, int R, int C);
/* T[M, R] = scale * X[M, K] . A[R, K]^T; X and A rows contiguous along K (K % 8 == 0); T may be a column slice of a wider buffer */
int vila_lora_down_bf16(const void* X, int64_t ldx, const void* A, int64_t lda, void* T, int64_t ldt, int M, int K, int R, float scale,
                        void* workspace, size_t workspace_bytes, vila_stream_t stream);
/* Y[M, N] = Res[M, N] (nullable) + scale * T[M, R] . Bt[R, N]; Bt rows contiguous along N (N % 8 == 0); Y and Res may be column slices;
 * Res aliases nothing, Y is write-only */
int vila_lora_up_bf16(const void* T, int64_t ldt, const void* Bt, int64_t ldb, const void* Res, int64_t ldres, void* Y, int64_t ldy, int M,
                      int N, int R, float scale, void* workspace, size_t workspace_bytes, vila_stream_t stream);
/* G[R, C] = scale * L[M, R]^T . X[M, C] (accumulate: + G); the contraction runs over the M rows and both operands are read as they lie
 * (C % 8 == 0, any M >= 1) */
int vila_lora_wgrad_bf16(const void* L, int64_t ldl, const void* X, int64_t ldx, void* G, int64_t ldg, int M, int R, int C, float scale,
                         int accumulate, void* workspace, size_t workspace_bytes, vila_stream_t stream);


/* ------------------------------------------------------------------------------------------------------------
 * The whole SFT forward + backward as ONE call — replaces what autograd does under the reference's
 * patched `Trainer.training_step` (llava/train/transformer_normalize_monkey_patch.py:183-249): LlavaLlamaModel.forward
 * (llava_llama.py:94-159) on a packed batch, loss = sum CE * loss_scale (loss_scale = 1 / GLOBAL num_items, :261-268), gradients of
 * every parameter of the LLM, the mm_projector and the vision tower.
 *   - weights / gradients: the inference structs; `*_grad` mirrors the weight struct with pointers to the bf16 gradient tensors of
 *     the same shapes (q/k/v fused like the weights).  The caller ZEROES the gradient buffers before the call (embedding rows are
 *     scatter-added; parameters the path never touches keep zero).  Every other gradient tensor is overwritten.
 *   - VilaSftBatch: the integer work of `_embed` / `repack_multimodal_data` (llava_arch.py:412-490, 744-800) planned on the host
 *     (vila_amd/host.py), all index arrays on the device
 *   - workspace: saved activations + temporaries (vila_sft_workspace_bytes; about 4 GB per 769-token sample at NVILA-8B), no
 *     re-computation
 *   - cb: called on the HOST, on the calling thread, right after the last kernel that writes a gradient bucket has been enqueued on
 *     `stream` (buckets in backward order: LM_HEAD (untied head only), FINAL_NORM, LLM_LAYER n-1..0, EMBED, PROJECTOR, VIT_LAYER n-1..0,
 *     VIT_EMBED).  That is where a data-parallel caller records an event and starts the bucket's all-reduce / optimizer on its own
 *     streams; nullable.
 * ------------------------------------------------------------------------------------------------------------ */
enum { VILA_BUCKET_LM_HEAD = 0, VILA_BUCKET_FINAL_NORM = 1, VILA_BUCKET_LLM_LAYER = 2, VILA_BUCKET_EMBED = 3, VILA_BUCKET_PROJECTOR = 4,
       VILA_BUCKET_VIT_LAYER = 5, VILA_BUCKET_VIT_EMBED = 6 };
typedef void (*VilaGradReadyCb)(void* arg, int bucket, int index);
typedef struct {
    const void* pixels; int n_images;                 /* [n_images, C, image, image] bf16 */
    int total_tokens;                                  /* T: tokens of the packed row */
    const int32_t* txt_src; const int32_t* txt_dst; int n_txt;       /* embed_tokens row (token id) -> packed row */
    const int32_t* feat_src; const int32_t* feat_dst; int n_feat;    /* mm_projector output row -> packed row */
    const int32_t* nl_src; const int32_t* nl_dst; int n_nl;          /* the "\n" end token of every image (ids) -> packed row */
    const int32_t* positions;                          /* [T] restarted per sample (llava_arch.py:751) */
    const int32_t* cu_seqlens; int n_seq; int max_seqlen;            /* flash-attn varlen description (model/utils/packing.py:12-21) */
    const int32_t* target_rows; const int64_t* targets; int n_targets;  /* packed rows that predict a label, and the labels */
    float loss_scale;
    /* dynamic_s2 recipe (scripts/NVILA/stage1_9tile.sh:19-22; llava_arch.py:298-390): s2_n_blocks > 0 => `pixels` holds the n_images TILES
     * of every scale of every image, the tower output goes through vila_s2_merge_bf16 (s2_desc, device [s2_n_blocks][6]) into the
     * projector (in_dim = n_scales * tower hidden, s2_n_blocks inputs), feat_src indexes the projector's [s2_n_blocks * tokens] rows
     * (the final chessboard merge is folded into it by the host plan), and the backward runs vila_s2_merge_bwd_bf16 (s2_tile_desc,
     * device [n_images][8]).  s2_n_blocks = 0: the plain single-scale path (the fields are ignored). */
    const int32_t* s2_desc; const int32_t* s2_tile_desc; int s2_n_blocks; int s2_n_scales; int32_t s2_splits[4];
    /* pooling video encoder (TSPVideoEncoder, encoders/video/tsp.py:28-52).  n_pools > 0 => behind the projector's rows the step keeps
     * n_media_rows - (projector rows) POOLED rows: pools = HOST array [n_pools][7] = {first projector input of the video's frames, n_frames,
     * pool_t, pool_h, pool_w, first row of this (video, pool size)'s pooled rows in the buffer, their count}; forward = vila_video_pool_bf16
     * per entry, backward = vila_video_pool_bwd_bf16 accumulated onto the frames' projector rows.  feat_src then indexes the whole buffer
     * [projector rows | pooled rows].  n_pools = 0: feat_src indexes the projector rows only (n_media_rows is ignored). */
    const int32_t* pools; int n_pools; int n_media_rows;
} VilaSftBatch;
size_t vila_sft_workspace_bytes(const VilaVitWeights* vit, const VilaProjWeights* proj, const VilaLlmWeights* llm, const VilaSftBatch* batch);
int vila_sft_fwd_bwd(const VilaVitWeights* vit, const VilaVitWeights* vit_grad, const VilaProjWeights* proj, const VilaProjWeights* proj_grad,
                     const VilaLlmWeights* llm, const VilaLlmWeights* llm_grad, const VilaSftBatch* batch, float* loss_out /* device */,
                     void* workspace, size_t workspace_bytes, VilaGradReadyCb cb, void* cb_arg, vila_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * dynamic_s2 multi-scale path — replaces merge_features_for_dynamic_s2 + split_chessboard +
 * rearrange of LlavaMetaModel.encode_images (llava/model/llava_arch.py:298-379):
 *   feats [n_tiles, g*g, C] (tower output for every tile of every image, scales in ascending order per image)
 *   desc  device [n_blocks][6] = {first tile of the image, bh | obh << 16, bw | obw << 16, block row i, block col j, single (block_sizes None)}
 *         bh x bw = tiles of the image's last scale; obh x obw = its OUTPUT blocks: 0 in the high halves = the same grid
 *         (s2_resize_output_to_scale_idx = -1, every shipped recipe); s x s for an earlier scale of s x s tiles (llava_arch.py:340-358)
 *   out   [n_blocks, g*g, n_scales*C] = the projector input.  splits[k] = scales[k] / scales[0] for k < n_scales-1 [host].
 * ------------------------------------------------------------------------------------------------------------ */
int vila_s2_merge_bf16(const void* feats, void* out, const int32_t* desc, int n_blocks, int grid, int channels, int n_scales,
                       const int32_t* splits, vila_stream_t stream);
/* Backward of the above for the SFT step of the dynamic_s2 recipe (autograd through llava_arch.py:298-379: F.interpolate(mode="area")
 * backward = dy / |window| broadcast into each scale's chessboard, merge / split_chessboard adjoints), as one gather:
 *   dy [n_blocks, g*g, n_scales*C] -> dx [n_tiles, g*g, C] (every element written, no accumulation)
 *   tile_desc device [n_tiles][8] = {first output block of the tile's image, bh | obh << 16, bw | obw << 16, scale index, tile row, tile col, single, 0} */
int vila_s2_merge_bwd_bf16(const void* dy, void* dx, const int32_t* tile_desc, int n_tiles, int grid, int channels, int n_scales,
                           const int32_t* splits, vila_stream_t stream);


/* ------------------------------------------------------------------------------------------------------------
 * Video encoders — replaces `pool` + `_process_features` of TSPVideoEncoder
 * (llava/model/encoders/video/tsp.py:10-11,28-52) and `_process_features` of BasicVideoEncoder (video/basic.py:30-41):
 *   feats [n_frames, grid*grid, C] bf16 (projected frames of ONE video) ->
 *   out   [(n_frames/pool_t) * (n_start + (grid/pool_h)*(grid/pool_w) + n_end), C]: per pooled frame the start-token rows, the mean over
 *   every (pool_t, pool_h, pool_w) window (fp32 accumulate), the end-token rows.  pool = (1,1,1) is BasicVideoEncoder.
 *   A ragged split (a pooled dimension not divisible by its pool size) is an error, as the reference's view() raises.
 * ------------------------------------------------------------------------------------------------------------ */
int vila_video_pool_bf16(const void* feats, void* out, int n_frames, int grid, int channels, int pool_t, int pool_h, int pool_w,
                         const void* start_rows, int n_start, const void* end_rows, int n_end, vila_stream_t stream);
/* Adjoint of the pooling for the SFT step (row a13 over a7; the `mean` backward of tsp.py:10-11 under autograd):
 *   dpooled [(n_frames/pool_t) * (grid/pool_h)(grid/pool_w), C] (gradient of the pooled FEATURE rows only) ->
 *   dfeats  [n_frames, grid*grid, C]: dfeats[t][h][w] = dpooled[t/pool_t][h/pool_h][w/pool_w] / (pool_t pool_h pool_w);
 *   accumulate != 0 adds into dfeats (the second and later pool sizes of one video). */
int vila_video_pool_bwd_bf16(const void* dpooled, void* dfeats, int n_frames, int grid, int channels, int pool_t, int pool_h, int pool_w,
                             int accumulate, vila_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * W4A16 decode (BASELINE configs[4]).  The reference's W4A16 backend is the external TinyChat
 * (README.md:87), with no code in-tree: the packed format is defined in vila_amd/csrc/gemv_w4.hip and produced by
 * vila_amd/quant.py; parity is against a CPU dequantise-then-fp32 oracle of the same quantised weights.
 *   w = (q - zero) * scale, uint4 q, groups of 128 along K.  Tile-major HBM layout (16-row tiles, one 1-KB wave load per group):
 *   Wq  [N/16][K/128][64 lanes][4] u32   lane = 16*g + n holds k = 128*group + 32*g + (0..31) of row n; per u32 nibble p<4 = element 2p,
 *                                        nibble p+4 = element 2p+1
 *   Wsz [N/16][K/128][16] u32            {bf16 scale, bf16 128 + zero}
 *   Row order inside a matrix: o/down as the bf16 weight; gate/up interleaved (row 2i = gate i, 2i+1 = up i); q and k heads of
 *   the fused qkv interleaved so RoPE partners are neighbours (row 2i = element i, 2i+1 = element i + head_dim/2), v heads as is.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
    const void *qkv_q, *qkv_sz, *o_q, *o_sz, *gateup_q, *gateup_sz, *down_q, *down_sz;
} VilaLlmLayerW4;
/* N outputs.  mode 0: y = W x (+bias)(+residual); mode 1: W holds 2N interleaved gate/up rows, y = silu(Wg x) * (Wu x);
 * optional fused RMSNorm on x.  K % 128 != 0 -> -1 */
int vila_gemv_w4_bf16(const void* x, const void* norm_w, float eps, const void* Wq, const void* Wsz,
                      const void* bias, const void* residual, void* y, int N, int K, int mode, vila_stream_t stream);
/* same contract as vila_llm_decode_step; `w` still supplies embed, norms, q/k/v biases and the bf16 lm_head */
int vila_llm_decode_step_w4(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host]*/, const VilaKvCache* cache,
                            const VilaDecodeState* st, void* workspace, size_t workspace_bytes, vila_stream_t stream);
/* the same step with a stochastic pick (generate(do_sample=True) on the quantised decoder): temperature -> top-k -> top-p -> draw */
int vila_llm_decode_step_w4_sample(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host]*/, const VilaKvCache* cache,
                            const VilaDecodeState* st, void* workspace, size_t workspace_bytes, const VilaSampling* sampling, vila_stream_t stream);

/* W4A16 batched decode GEMV (vila_amd/csrc/gemv_w4_batch.hip) on the same packed buffers: y[m][N] = x[m][K] . W^T for the 1 <= n <= 16 rows of
 * x (row stride ldx, a multiple of 8 elements); y and residual have row stride N.  mode 0: (+bias)(+residual; y may alias it); mode 1: W holds
 * 2N interleaved gate/up rows, y = silu(Wg x) * (Wu x), bias and residual must be NULL.  Deterministic (fixed reduction order, no atomics);
 * rows >= n and columns >= N of y are not written.  n outside 1..16, K % 128 != 0 or another mode -> -1. */
int vila_gemv_w4_batch_bf16(const void* x, int64_t ldx, int n, const void* Wq, const void* Wsz, const void* bias, const void* residual,
                            void* y, int N, int K, int mode, vila_stream_t stream);
/* The bf16 skinny GEMM of the batched decode, verify and shared-prefix steps (vila_amd/csrc/decode_batch.hip, bgemm_dma_kernel) on the caller's
 * buffers, as those steps launch it.  x: 1 <= n <= 16 rows of K bf16 (row stride ldx, a multiple of 8 elements; x and W 16-byte aligned); W, W2:
 * [N][K] bf16 with row stride K; K a positive multiple of 64, any N > 0.
 * vila_gemm_batch_bf16: W2 == NULL: y[m][N] = x[m] . W^T (+bias); the fp32 sum goes to y_f32 (row stride ldf) and/or, rounded to bf16, to y (row
 *   stride ldy), where `residual` (row stride ldr; may be y itself) is added to the rounded value and the sum rounded again.  At least one output.
 *   W2 != NULL (gate/up): y = bf16(silu(bf16(x . W^T))) * bf16(x . W2^T); bias, residual and y_f32 must be NULL.
 * vila_qkv_batch_bf16: Wqkv holds (q_heads + 2 kv_heads) * head_dim rows, q | k | v; head_dim % 32 == 0.  Row m gets bias, then rotate-half RoPE on
 *   its q and k heads with rope_cs[m][0 : head_dim/2] = cos, [head_dim/2 : head_dim] = sin (fp32); q goes to q_out[m] (row stride ldq), K and V
 *   to row pos[m] of kcache / vcache + m * slot_stride, each [kv_heads][max_ctx][head_dim]; a row with pos[m] >= max_ctx writes q and no K/V.
 * Deterministic; rows >= n, columns >= N and every other cache row are not written.  Every refusal (-1) comes before anything is launched. */
int vila_gemm_batch_bf16(const void* x, int64_t ldx, int n, const void* W, const void* W2, const void* bias, const void* residual, int64_t ldr,
                         void* y, int64_t ldy, float* y_f32, int64_t ldf, int N, int K, vila_stream_t stream);
int vila_qkv_batch_bf16(const void* x, int64_t ldx, int n, const void* Wqkv, const void* bias, void* q_out, int64_t ldq, void* kcache, void* vcache,
                        int64_t slot_stride, const int32_t* pos, const float* rope_cs, int q_heads, int kv_heads, int head_dim, int max_ctx, int K,
                        vila_stream_t stream);
/* The fused q|k|v projections of the W4A16 decode steps on the caller's buffers, as those steps launch them (tests/test_gpu_w4_elements.py).
 * Wq / Wsz: the packed (q_heads + 2 kv_heads) * head_dim rows of a layer's fused q|k|v matrix, q and k heads RoPE-interleaved (above);
 * head_dim % 16 == 0, K % 128 == 0; bias [N] in natural q | k | v order or NULL; rope_cs fp32, cos | sin.
 * vila_qkv_w4_bf16 (gemv_w4.hip mode 3, the solo step's): x [K] with an optional fused RMSNorm (norm_w NULL: none); RoPE from rope_cs[head_dim];
 *   q goes to q_out [q_heads * head_dim], K and V to row *pos (device int32) of kcache / vcache [kv_heads][max_ctx][head_dim]; *pos >= max_ctx
 *   writes q and no K/V.
 * vila_qkv_w4_batch_bf16 (gemv_w4_batch.hip mode 2): the arguments of vila_qkv_batch_bf16 with Wq / Wsz in place of Wqkv, same contract.
 * Deterministic; nothing else is written.  Every refusal (-1) comes before anything is launched. */
int vila_qkv_w4_bf16(const void* x, const void* norm_w, float eps, const void* Wq, const void* Wsz, const void* bias, void* q_out,
                     void* kcache, void* vcache, const int32_t* pos, const float* rope_cs, int q_heads, int kv_heads, int head_dim,
                     int max_ctx, int K, vila_stream_t stream);
int vila_qkv_w4_batch_bf16(const void* x, int64_t ldx, int n, const void* Wq, const void* Wsz, const void* bias, void* q_out, int64_t ldq,
                           void* kcache, void* vcache, int64_t slot_stride, const int32_t* pos, const float* rope_cs, int q_heads, int kv_heads,
                           int head_dim, int max_ctx, int K, vila_stream_t stream);
/* vila_llm_decode_step_batch with the q|k|v, o, gate/up and down projections of every layer read from `qlayers` [host] (W4A16 batched GEMVs).
 * `w` still supplies embed, norms, the q/k/v biases (one contiguous q|k|v vector) and the bf16 lm_head; its projection pointers are not read.
 * Same contract and limits as vila_llm_decode_step_batch (head_dim 128, max_ctx <= 2048, or <= 32768 with the _ctx workspace, 1 <= n <= min(16, n_slots), q_heads * head_dim ==
 * hidden), plus hidden % 128 == 0 and intermediate % 128 == 0; each is checked before anything is launched (-1). */
size_t vila_llm_decode_batch_w4_workspace_bytes(const VilaLlmShape* s, int n);
size_t vila_llm_decode_batch_w4_workspace_bytes_ctx(const VilaLlmShape* s, int n, int max_ctx);
int vila_llm_decode_step_batch_w4(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host]*/, const VilaKvCache* cache,
                                  const VilaDecodeBatch* st, void* workspace, size_t workspace_bytes, vila_stream_t stream);
/* the W4 batched step with the per-row pick of vila_llm_decode_step_batch_sample */
size_t vila_llm_decode_batch_w4_sample_workspace_bytes(const VilaLlmShape* s, int n);
size_t vila_llm_decode_batch_w4_sample_workspace_bytes_ctx(const VilaLlmShape* s, int n, int max_ctx);
int vila_llm_decode_step_batch_w4_sample(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host]*/, const VilaKvCache* cache,
                                         const VilaDecodeBatch* st, void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp,
                                         vila_stream_t stream);
/* the W4 steps of a session with a shared prompt prefix (VilaDecodePrefix) */
size_t vila_llm_decode_batch_prefix_w4_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx);
size_t vila_llm_decode_batch_prefix_w4_sample_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx);
int vila_llm_decode_step_batch_prefix_w4(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host]*/, const VilaKvCache* cache,
                                         const VilaDecodeBatch* st, const VilaDecodePrefix* prefix, void* workspace, size_t workspace_bytes,
                                         vila_stream_t stream);
int vila_llm_decode_step_batch_prefix_w4_sample(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host]*/, const VilaKvCache* cache,
                                                const VilaDecodeBatch* st, const VilaDecodePrefix* prefix, void* workspace, size_t workspace_bytes,
                                                const VilaBatchSampling* sp, vila_stream_t stream);
/* vila_llm_decode_step_verify with the four projections of every layer read from `qlayers`; workspace of vila_llm_decode_verify_workspace_bytes */
int vila_llm_decode_step_verify_w4(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host]*/, const VilaKvCache* cache,
                                   const VilaDecodeVerify* st, void* workspace, size_t workspace_bytes, vila_stream_t stream);
/* vila_llm_decode_step_verify_sample likewise; workspace of vila_llm_decode_verify_sample_workspace_bytes, `sp` of ONE entry per array */
int vila_llm_decode_step_verify_w4_sample(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host]*/, const VilaKvCache* cache,
                                          const VilaDecodeVerify* st, void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp,
                                          vila_stream_t stream);

/* W4A16 prefill GEMM (vila_amd/csrc/gemm_w4.hip) on the same packed buffers: y[M][N] = x[M][K] . W^T, x bf16 row stride K, y row stride N,
 * any M >= 1.  mode 0: (+bias)(+residual, row stride N; y may alias it); mode 1: W holds 2N interleaved gate/up rows, y = silu(Wg x) * (Wu x),
 * bias and residual must be NULL.  Deterministic (K-sliced grids add their fp32 slices in a fixed order).  K % 128 != 0, N % 16 != 0, another
 * mode or a bias / residual the mode does not take -> -1.
 * workspace: vila_gemm_w4_workspace_bytes(M, N, K, mode) bytes (0: none needed, NULL accepted). */
size_t vila_gemm_w4_workspace_bytes(int M, int N, int K, int mode);
int vila_gemm_w4_bf16(const void* x, const void* Wq, const void* Wsz, const void* bias, const void* residual, void* y,
                      int M, int N, int K, int mode, void* workspace, size_t workspace_bytes, vila_stream_t stream);
/* the fused q|k|v projection of a W4 layer (rows of the first q_heads + kv_heads heads RoPE-interleaved, VilaLlmLayerW4.qkv_q): y [M][(q_heads
 * + 2 kv_heads) head_dim] in natural column order with the bias added, as the bf16 q|k|v GEMM leaves it for RoPE.  Workspace: mode 2 above. */
int vila_gemm_w4_qkv_bf16(const void* x, const void* Wq, const void* Wsz, const void* bias, void* y, int M, int q_heads, int kv_heads,
                          int head_dim, int K, void* workspace, size_t workspace_bytes, vila_stream_t stream);
/* vila_llm_prefill with the five decoder projections read from the int4 layers (`w` still supplies embed, norms, q/k/v biases, lm_head;
 * its projection pointers are not read).  Same arguments and contract, `qlayers` [host] added; the pruned last layer runs the W4 GEMVs. */
size_t vila_llm_prefill_w4_workspace_bytes(const VilaLlmShape* s, int total_tokens);
int vila_llm_prefill_w4(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host]*/, const void* embeds, const int32_t* positions,
                        const int32_t* cu_seqlens, int n_seq, int total_tokens, int max_seqlen, const int32_t* seq_of_tok, const VilaKvCache* cache,
                        const int32_t* last_rows, int n_last, float* last_logits, float* all_logits, void* final_hidden,
                        void* layer_hidden, void* workspace, size_t workspace_bytes, vila_stream_t stream);

/* Prefill onto a live KV cache: T tokens of ONE sequence appended to `slot` of `cache`, which holds `past` positions.  The tokens take positions
 * past .. past + T - 1, their K / V are written there (no other row of the cache is touched), and every row attends the slot's keys 0 .. its own
 * position.  `past` is a host integer (a prefill is never graph-captured).  Outputs as vila_llm_prefill: last_rows / last_logits, final_hidden
 * [T, hidden], layer_hidden [(n_layers+1), T, hidden], rows counted inside these T tokens.  head_dim 128 and q_heads * 128 == hidden;
 * past + T <= cache->max_ctx; 0 <= slot < cache->n_slots; anything else is refused before a launch.  The _w4 form reads the five decoder
 * projections from the int4 layers like vila_llm_prefill_w4. */
size_t vila_llm_prefill_append_workspace_bytes(const VilaLlmShape* s, int T);
size_t vila_llm_prefill_append_w4_workspace_bytes(const VilaLlmShape* s, int T);
int vila_llm_prefill_append(const VilaLlmWeights* w, const void* embeds, int T, int past, int slot, const VilaKvCache* cache,
                            const int32_t* last_rows, int n_last, float* last_logits, void* final_hidden, void* layer_hidden,
                            void* workspace, size_t workspace_bytes, vila_stream_t stream);
int vila_llm_prefill_append_w4(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host]*/, const void* embeds, int T, int past, int slot,
                               const VilaKvCache* cache, const int32_t* last_rows, int n_last, float* last_logits, void* final_hidden,
                               void* layer_hidden, void* workspace, size_t workspace_bytes, vila_stream_t stream);

/* Repetition, presence and frequency penalties in front of the token choice (vila_amd/csrc/penalty.hip): the first element of HF's processor chain,
 * ahead of temperature -> top-k -> top-p.  Row r keeps counts[r][vocab] (uint16, rows ld_counts apart): how often its request has GENERATED each id.
 * The table is zero when a request starts (the host's duty), saturates at 65535 and never counts the prompt.  One launch, per row r and index i:
 *   bump        counts[r][token[r]] += 1 for the token the step consumes (token NULL or an id outside 0 .. vocab - 1: nothing), before the count is used
 *   repetition  c > 0: y = x < 0 ? x * rep : x / rep               (HF RepetitionPenaltyLogitsProcessor)
 *   frequency   y = y - freq * (float)c                            (OpenAI's definition, vLLM's order)
 *   presence    c > 0: y = y - pres
 * each ONE correctly rounded fp32 operation, so y is bit for bit the same expression in torch on the CPU and rep = 1, pres = freq = 0 return x's bits.
 * All members are DEVICE arrays read at run time (the three parameters hold one entry per row): one captured hipGraph serves any values. */
typedef struct {
    const float* repetition;    /* [n]; > 0 (the host checks) */
    const float* presence;      /* [n] */
    const float* frequency;     /* [n] */
    uint16_t* counts;           /* [n][ld_counts] */
    int64_t ld_counts;          /* >= vocab */
} VilaPenalties;
/* The operator: logits [n][ld] fp32 -> out [n][ld_out] fp32 (nothing at or beyond vocab is read or written); pick_v / pick_i (both or neither)
 * [n][vila_logits_penalize_slices()]: per slice of a processed row its maximum and the first index that holds it. */
int vila_logits_penalize_slices(void);
int vila_logits_penalize_f32(const float* logits, int64_t ld, int n, int vocab, const VilaPenalties* pen, const int64_t* token /*nullable: no bump*/,
                             float* out, int64_t ld_out, float* pick_v, int* pick_i /*nullable*/, vila_stream_t stream);
/* The decode steps with that launch between the logits and the pick: st->logits stays the raw model logits, the pick (greedy: first index of the
 * maximum; sampled: the sampler of the plain step, unchanged) runs on the processed row, and token[] is counted before it is replaced.  One entry
 * per driver: qlayers NULL = bf16, else the W4 step; sp NULL = greedy; prefix NULL = a plain batch session.  The launches in front of the pick are
 * the plain steps', so the logits are the same bits.  Workspaces: the sizes below (they differ from the plain steps').  The verify steps' penalised
 * form is vila_llm_decode_step_verify_processed (below). */
size_t vila_llm_decode_penalized_workspace_bytes(const VilaLlmShape* s, int max_ctx);
int vila_llm_decode_step_penalized(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host], nullable*/, const VilaKvCache* cache,
                                   const VilaDecodeState* st, void* workspace, size_t workspace_bytes, const VilaSampling* sp /*nullable*/,
                                   const VilaPenalties* pen, vila_stream_t stream);
size_t vila_llm_decode_batch_penalized_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx, int prefix);
int vila_llm_decode_step_batch_penalized(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host], nullable*/, const VilaKvCache* cache,
                                         const VilaDecodeBatch* st, const VilaDecodePrefix* prefix /*nullable*/, void* workspace, size_t workspace_bytes,
                                         const VilaBatchSampling* sp /*nullable*/, const VilaPenalties* pen, vila_stream_t stream);

/* Structured output: a token-level automaton per row in front of the token choice (vila_amd/csrc/constrain.hip), behind the penalties and ahead of
 * temperature -> top-k -> top-p (where HF runs a caller's logits_processor).  Row r carries a deterministic automaton over token CLASSES, compiled on
 * the host (vila_amd/constrain.py).  Per row r of one step:
 *   advance  s = state[r] >= 0 and the consumed token t = token[r] in 0 .. vocab - 1: s2 = next[r][s * C + cls[r][t]], C = n_classes[r]; s2 >= 0
 *            replaces the state, otherwise it stays.  token NULL or an id out of range: no advance (the first token is masked from the start state).
 *   mask     y[i] = next[r][state * C + cls[r][i]] >= 0 ? x[i] : -inf for every i < vocab; a row with state -1 copies x bit for bit.
 * Nothing at or beyond vocab is read or written; out may alias logits.  All members are DEVICE arrays read at run time: one captured hipGraph serves
 * any automata.  The kernel cannot validate their contents (the host binds them); it keeps its own reads inside a row's table and treats a class
 * >= C as not allowed. */
#define VILA_CONSTRAIN_MAX_CLASSES 4096
typedef struct {
    int32_t*        state;      /* [n] device; -1 = the row is unconstrained; else the row's current state */
    const uint16_t* cls;        /* [n][ld_cls] class of every token id under the row's automaton, ld_cls >= vocab */
    int64_t         ld_cls;
    const int16_t*  next;       /* [n][ld_next]: the row's table, row-major [n_states][n_classes[r]]; < 0 = not allowed in that state */
    int64_t         ld_next;
    const int32_t*  n_classes;  /* [n]; 1 .. VILA_CONSTRAIN_MAX_CLASSES */
} VilaConstraints;
/* The operator: logits [n][ld] fp32 -> out [n][ld_out] fp32; pick_v / pick_i (both or neither) [n][vila_logits_constrain_slices()]: per slice of a
 * processed row its maximum and the first index that holds it (an all -inf row merges to index 0).  n in 1..65535. */
int vila_logits_constrain_slices(void);
int vila_logits_constrain_max_classes(void);
int vila_logits_constrain_f32(const float* logits, int64_t ld, int n, int vocab, const VilaConstraints* con, const int64_t* token /*nullable: no advance*/,
                              float* out, int64_t ld_out, float* pick_v, int* pick_i /*nullable*/, vila_stream_t stream);
/* The decode steps with raw logits -> penalties (if pen) -> constrain -> pick.  st->logits stays raw; the launches in front of the pick are the plain
 * steps', so the logits are the same bits.  qlayers, sp, prefix and pen are nullable, as in the penalised entries, whose workspace sizes these share.
 * The verify steps' constrained form is vila_llm_decode_step_verify_processed (below). */
size_t vila_llm_decode_constrained_workspace_bytes(const VilaLlmShape* s, int max_ctx);
int vila_llm_decode_step_constrained(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host], nullable*/, const VilaKvCache* cache,
                                     const VilaDecodeState* st, void* workspace, size_t workspace_bytes, const VilaSampling* sp /*nullable*/,
                                     const VilaPenalties* pen /*nullable*/, const VilaConstraints* con, vila_stream_t stream);
size_t vila_llm_decode_batch_constrained_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx, int prefix);
int vila_llm_decode_step_batch_constrained(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host], nullable*/, const VilaKvCache* cache,
                                           const VilaDecodeBatch* st, const VilaDecodePrefix* prefix /*nullable*/, void* workspace, size_t workspace_bytes,
                                           const VilaBatchSampling* sp /*nullable*/, const VilaPenalties* pen /*nullable*/, const VilaConstraints* con,
                                           vila_stream_t stream);

/* Any top_k for the rows of the batched sampler (opt-in; vila_amd/csrc/sample.hip): the entries above serve top_k in 1..64 and clamp anything else;
 * the entries below also serve top_k = 0 (no top-k filter, HF's meaning: pure top-p sampling) and top_k > 64, per row and from the same device
 * arrays, so ONE captured hipGraph serves any mix of greedy rows, rows of 1..64 and such rows.  One launch more, of one 1024-thread block per row,
 * draws every row with temperature > 0 and (top_k == 0 or top_k > 64) by the exact selection of vila_sample_f32 — the predicate by which that
 * function picks its own path — and every other block of it returns at once.  The contract of VilaBatchSampling extends to them: a sampled row's
 * token is bit for bit what vila_sample_f32 returns for the same logits row, parameters, seed and counter, for every top_k >= 0.  A negative
 * top_k is still clamped to 1 and top_p to (0, 1].
 * vila_sample_batch_any_f32: vila_sample_batch_f32 with that launch (four launches whatever n; the workspace of vila_sample_batch_workspace_bytes).
 * dist_out (nullable) [n][128] as there; a row drawn by the exact path gets zeros and -1 ids.  dense_out (nullable) [n][ld_dense], ld_dense >= vocab:
 * such a row's distribution over the vocabulary (what vila_sample_f32 returns in dist_out for it); the other rows' entries are not written. */
int vila_sample_batch_any_f32(const float* logits, int64_t ld_logits, int n, int vocab, const VilaBatchSampling* sp, const int32_t* counter,
                              int64_t* out, void* workspace, float* dist_out /*nullable*/, float* dense_out /*nullable*/, int64_t ld_dense,
                              vila_stream_t stream);
/* The sampled batched step with that pick.  One entry: qlayers NULL = bf16, else the W4 step; prefix NULL = a plain batch session; pen / con NULL =
 * no penalties / no automata in front of the pick; sp is required.  One workspace size serves every combination.  The launches in front of the pick
 * are the plain steps', so st->logits stays raw and keeps the same bits. */
size_t vila_llm_decode_batch_any_k_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx, int prefix);
int vila_llm_decode_step_batch_any_k(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host], nullable*/, const VilaKvCache* cache,
                                     const VilaDecodeBatch* st, const VilaDecodePrefix* prefix /*nullable*/, void* workspace, size_t workspace_bytes,
                                     const VilaBatchSampling* sp, const VilaPenalties* pen /*nullable*/, const VilaConstraints* con /*nullable*/,
                                     vila_stream_t stream);
/* The sampled verify step with that pick: `sp` of ONE entry per array, read by every row; workspace of vila_llm_decode_verify_sample_workspace_bytes. */
int vila_llm_decode_step_verify_any_k(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host], nullable*/, const VilaKvCache* cache,
                                      const VilaDecodeVerify* st, void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp,
                                      vila_stream_t stream);

/* Log-probabilities of the chosen token and of its top alternatives (vila_amd/csrc/logprob.hip): the `logprobs` / `top_logprobs` of an OpenAI-style
 * endpoint, HF's `compute_transition_scores`.  For a row x[0 .. vocab - 1] of RAW fp32 logits, all in fp32:
 *   M = max x,  lse = M + log(sum_i exp(x_i - M)),  logprob(t) = x_t - lse          (an -inf entry contributes 0 to the sum)
 * RAW: the numbers describe the model's own distribution.  Temperature, top-k, top-p and penalties do not enter, also where the session's pick is
 * sampled or penalised (st->logits stays raw under every step entry).
 * The alternatives are the top_n (0 .. VILA_LOGPROBS_MAX_TOP) largest raw logits in descending order, ties towards the LOWER index, selected by
 * comparing the floats only: the ids are exact.  Places from top_n on, and places that a vocabulary below 20 cannot fill, hold id -1 and logprob
 * -inf.  The chosen token's logprob is always reported; a token outside 0 .. vocab - 1 gives NaN for it and disturbs nothing else.
 * Two launches whatever n; every reduction runs in a fixed order without floating-point atomics, so the bits are the same on every run, and a row's
 * bits depend neither on n nor on which row it is.  Nothing at or beyond vocab within a row is read.
 * Records: row r writes record rec[r] + rec_bias (rec NULL: rec_bias); an index outside 0 .. max_rec - 1 writes NOTHING.  token, rec and the logits
 * are device arrays read at run time: one captured hipGraph serves every request.
 * Behind a decode step: launch it AFTER the step entry on the same stream, with logits = st->logits, token = st->token, rec = st->n_out and
 * rec_bias = -1.  It then records the token that step chose, and record k of a row lines up with out_ids[k] (an idle row that has stepped past
 * max_out writes nothing, as out_ids is guarded).  A verify step emits up to n tokens of ONE sequence: its records are written by
 * vila_llm_decode_step_verify_processed (below), through the one-sequence mode vila_logprobs_seq_f32. */
#define VILA_LOGPROBS_MAX_TOP 20
typedef struct {
    float*   token_logprob;   /* [n][max_rec] */
    float*   top_logprob;     /* [n][max_rec][VILA_LOGPROBS_MAX_TOP]; NULL together with top_id: no alternatives (top_n must be 0) */
    int32_t* top_id;          /* same shape */
    int      max_rec;         /* >= 1 */
} VilaLogprobOut;
size_t vila_logprobs_workspace_bytes(int n);
/* the number of logits in one slice of a row of `vocab` entries (stage 1 reduces a row slice by slice; a multiple of 4) */
int vila_logprobs_slice_width(int vocab);
/* n >= 1 rows (not limited to 16), ld >= vocab; workspace: vila_logprobs_workspace_bytes(n) bytes, 8-byte aligned.  Bad arguments are refused before
 * any launch. */
int vila_logprobs_f32(const float* logits, int64_t ld, int n, int vocab, const int64_t* token /*[n] device*/, int top_n /*0..20*/,
                      const int32_t* rec /*[n] device, nullable: record 0*/, int rec_bias, const VilaLogprobOut* out,
                      void* workspace, vila_stream_t stream);


/* Speculative decoding for penalised, constrained and logprob requests: the verify step with the processing chain in front of its pick,
 *   raw logits -> penalties -> automaton mask -> pick (greedy) or draw (sampled, top_k 1..64 or, with any_k, every top_k >= 0) -> accept -> commit,
 * and the records of the tokens it emits.  A step runs n = k + 1 rows of ONE sequence; row i consumes token[i] at position pos + i, so it is processed
 * as the session drafting nothing processes the step that consumes token[i], after consuming token[0 .. i]:
 *   penalties  row i sees c_i(v) = min(65535, counts[v] + #{j <= i : token[j] == v}) (ids outside 0 .. vocab - 1 count nothing): the saturating sum,
 *              which equals the sequential saturating bumps.  y = the expression of VilaPenalties with c_i(v), one rounding per operation; neutral
 *              values return x's bits.  `pen` describes ONE sequence: one count row and ONE-entry parameter arrays read by every row (as `sp` is).  The
 *              launch does NOT write the table.
 *   automaton  s_0 = adv(state, token[0]), s_i = adv(s_{i-1}, token[i]) with adv the advance rule of VilaConstraints (a transition < 0, an id out of
 *              range or a class >= C leaves the state; -1 stays -1 and copies the row); row i is masked from s_i with the ONE cls / next table.  The launch
 *              does NOT write `state`.  A draft the automaton forbids holds -inf in the row in front of it and is rejected like any wrong draft.
 *   pick / draw, accept   the plain verify steps' launches, reading the processed rows; st->logits stays RAW; the draw of row i keeps counter pos + i.
 *   commit     behind the accept, with m = *n_accept, by one thread: counts[t] gets one saturating bump for each of the m + 1 tokens the step consumed
 *              (token[0 .. m] as they were before the accept replaced token[0]), in order, and state = s_m.  Nothing of the rows behind m reaches the
 *              table or the state.
 *   records    RAW (VilaLogprobOut of ONE sequence, n = 1 in its shapes): row i <= m emitted out_ids[old + i], old = *n_out - (m + 1) behind the accept,
 *              and writes record old + i; rows behind m and indices at or beyond max_rec (or max_out) write nothing.  Record k lines up with out_ids[k],
 *              with the bits vila_logprobs_f32 gives that row alone.  top_logprob / top_id non-NULL: all 20 alternatives.
 * A row's logits do not depend on the step it runs in, so the ids, the table, the state and the records are those of the same session drafting nothing.
 * qlayers NULL = bf16, else W4; sp NULL = greedy; any_k != 0 needs sp; pen, con and lp NULL = that stage is off, and with all three NULL the launches
 * are the plain verify step's.  One workspace size serves every combination.  Bad arguments are refused before any launch. */
size_t vila_llm_decode_verify_processed_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx);
int vila_llm_decode_step_verify_processed(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*[host], nullable*/, const VilaKvCache* cache,
                                          const VilaDecodeVerify* st, void* workspace, size_t workspace_bytes, const VilaBatchSampling* sp /*nullable*/,
                                          int any_k, const VilaPenalties* pen /*nullable*/, const VilaConstraints* con /*nullable*/,
                                          const VilaLogprobOut* lp /*nullable*/, vila_stream_t stream);
/* Its launches on their own.  n in 1..16 rows of ONE sequence, token [n] device.
 * penalise-verify: logits [n][ld] -> out [n][ld_out] with pen's ONE count row (read only) and entry 0 of its parameter arrays; pick_v / pick_i (both or
 *   neither) [n][vila_logits_penalize_slices()].
 * constrain-verify: the chain s_0 .. s_{n-1} of con's ONE automaton along token[] -> states_out [n] (con->state is read only), then logits -> out masked
 *   per row; pairs as above.  out may alias logits.
 * commit: consumed [n] (the tokens a step consumed), states [n] (the chain), *n_accept = m (clamped to 0 .. n - 1): counts bumped for consumed[0 .. m] where
 *   pen is given, con->state = states[m] where con is given (one of the two at least).
 * one-sequence records: vila_logprobs_f32 with every row writing output row 0: row r writes record rec[r] (required; outside 0 .. max_rec - 1: nothing) of
 *   token_logprob [max_rec], top_logprob / top_id [max_rec][20]. */
int vila_logits_penalize_verify_f32(const float* logits, int64_t ld, int n, int vocab, const VilaPenalties* pen, const int64_t* token, float* out,
                                    int64_t ld_out, float* pick_v, int* pick_i /*nullable*/, vila_stream_t stream);
int vila_logits_constrain_verify_f32(const float* logits, int64_t ld, int n, int vocab, const VilaConstraints* con, const int64_t* token,
                                     int32_t* states_out, float* out, int64_t ld_out, float* pick_v, int* pick_i /*nullable*/, vila_stream_t stream);
int vila_verify_commit(const VilaPenalties* pen /*nullable*/, const VilaConstraints* con /*nullable*/, int vocab, const int64_t* consumed,
                       const int32_t* states, const int32_t* n_accept, int n, vila_stream_t stream);
int vila_logprobs_seq_f32(const float* logits, int64_t ld, int n, int vocab, const int64_t* token /*[n] device*/, int top_n /*0..20*/,
                          const int32_t* rec /*[n] device*/, const VilaLogprobOut* out, void* workspace, vila_stream_t stream);

/* LoRA adapters served unmerged: a per-row adapter in the batched step (vila_amd/csrc/lora_decode.hip, decode_batch.hip).
 * A bank holds `capacity` (1 .. 32) slots of rank r (16, 32, 48 or 64; an adapter of lower rank is zero-padded) in buffers whose addresses never
 * change.  row_adapter [n] int32 (device) names each row's slot, or -1 for none (a value outside 0 .. capacity - 1 counts as -1); it is read at run
 * time, so ONE captured hipGraph serves every mix of rows and every load or unload.  Per layer and per stack of projections that share an input
 * (q|k|v: Rs = 3 r rows, N = (q + 2 kv) * head_dim columns; o: r, hidden; gate|up: 2 r, 2 * inter; down: r, hidden):
 *   A  [capacity][Rs][K] bf16          the members' lora_A stacked, rows contiguous along K
 *   B  [capacity][r / 8][N][8] bf16    lora_B of the members side by side over the stack's columns, chunk-major: element (c, col, e) = B[col][8 c + e]
 * and scale [capacity] fp32 = alpha / r_adapter.  A projection not targeted has zero B; zero rows and columns contribute exact zeros.
 * shrink: T[i][0 : Rs) = scale[a] * (x_i . A_a^T), a = row_adapter[i]; x [n <= 16][K] bf16 (ldx % 8 == 0, 16-byte aligned), K % 64 == 0, Rs % 16 == 0; T fp32.
 * expand: D[i][col] = sum_j T[i][seg(col) + j] * B_a[col][j], j = 0 .. r - 1 in that order (fmaf); seg = 0 for col < c1, r for col < c2, else 2 r
 *   (one member: c1 = c2 = N; two: c2 = N); fp32 out.
 * Both: a slot that no row names is not read; a row without an adapter gets +0.0; row i's T and D depend on x_i (T_i) and its slot only, bit for bit,
 * whatever n and the other rows; fixed summation order, no atomics; nothing outside [n][Rs] / [n][N] is written.  Refusals (-1) come before any launch. */
int vila_lora_shrink_bf16(const void* x, int64_t ldx, int n, const void* A, int64_t slot_stride /*elements*/, const float* scale,
                          const int32_t* row_adapter, int capacity, float* T, int64_t ldt, int Rs, int K, vila_stream_t stream);
int vila_lora_expand_f32(const float* T, int64_t ldt, int n, const void* B, int64_t slot_stride /*elements*/, const int32_t* row_adapter, int capacity,
                         float* D, int64_t ldd, int N, int r, int c1, int c2, vila_stream_t stream);
/* vila_gemm_batch_bf16 (W2 == NULL) / its gate/up form / vila_qkv_batch_bf16 with an fp32 addend [n][N] (gate/up: [n][2 N], gate | up; row stride lda)
 * added to the fp32 sum in front of the bias and the first rounding: so in front of silu (gate/up) and of RoPE and the cache append (q|k|v).  A row
 * with row_adapter[m] < 0 skips the add (it is NOT + 0.0: a sum of -0.0 keeps its sign) and has the bits of the entries without addend; row_adapter
 * NULL: every row adds.  addend NULL launches the very kernels of those entries. */
int vila_gemm_batch_lora_bf16(const void* x, int64_t ldx, int n, const void* W, const void* bias, const void* residual, int64_t ldr, void* y, int64_t ldy,
                              float* y_f32, int64_t ldf, int N, int K, const float* addend, int64_t lda, const int32_t* row_adapter, vila_stream_t stream);
int vila_gateup_batch_lora_bf16(const void* x, int64_t ldx, int n, const void* Wgate, const void* Wup, void* y, int64_t ldy, int N, int K,
                                const float* addend, int64_t lda, const int32_t* row_adapter, vila_stream_t stream);
int vila_qkv_batch_lora_bf16(const void* x, int64_t ldx, int n, const void* Wqkv, const void* bias, void* q_out, int64_t ldq, void* kcache, void* vcache,
                             int64_t slot_stride, const int32_t* pos, const float* rope_cs, int q_heads, int kv_heads, int head_dim, int max_ctx, int K,
                             const float* addend, int64_t lda, const int32_t* row_adapter, vila_stream_t stream);
typedef struct {
    const void *a_qkv, *b_qkv, *a_o, *b_o, *a_gateup, *b_gateup, *a_down, *b_down;   /* slot 0 of each buffer (layouts above) */
} VilaLoraBankLayer;
typedef struct {
    const VilaLoraBankLayer* layers;   /* [n_layers] host */
    const float*   scale;              /* [capacity] device */
    const int32_t* row_adapter;        /* [n] device */
    int32_t        capacity, r;
} VilaLoraBank;
/* The batched step with per-row adapters: in front of each of a layer's four projections, shrink and expand on the projection's own input (eight
 * small launches per layer), the result added in the GEMM's epilogue: a row computes round(acc + D + bias) with T and D in fp32.  lm_head is never
 * adapted.  ONE entry: sp, pen and con NULL = greedy / no penalties / no automata, any_k != 0 needs sp; logprobs run behind it as behind every step.
 * qlayers and prefix must be NULL: the step has no int4 and no shared-prefix form (-1), nor have the verify and solo steps an adapter form.  A row
 * with -1 keeps the bits of vila_llm_decode_step_batch. */
size_t vila_llm_decode_batch_lora_workspace_bytes(const VilaLlmShape* s, int n, int max_ctx, int r);
int vila_llm_decode_step_batch_lora(const VilaLlmWeights* w, const VilaLlmLayerW4* qlayers /*must be NULL*/, const VilaKvCache* cache,
                                    const VilaDecodeBatch* st, const VilaDecodePrefix* prefix /*must be NULL*/, const VilaLoraBank* bank, void* workspace,
                                    size_t workspace_bytes, const VilaBatchSampling* sp /*nullable*/, const VilaPenalties* pen /*nullable*/,
                                    const VilaConstraints* con /*nullable*/, int any_k, vila_stream_t stream);
/* The prefill with every packed sequence under ONE adapter, in the trainer's orientation (vila_amd/lora.py): per layer and stack the stacked
 * A [Rs][K] and the members' Bt side by side, [r][N] over the stack's N output columns (a projection that is not adapted: zero columns), rank r
 * (16, 32, 48 or 64), scale alpha / r_adapter.  Per projection lora_down on the stack's input, lora_up into the base GEMM's residual (t and u rounded
 * to bf16, the trainer's forward dataflow), RoPE and the norms as launches of their own, gate and up as two GEMMs and silu_mul; no last-row pruning.
 * The other arguments are vila_llm_prefill's. */
typedef struct {
    const void *a_qkv, *bt_qkv, *a_o, *bt_o, *a_gateup, *bt_gateup, *a_down, *bt_down;
} VilaLoraLayer;
size_t vila_llm_prefill_lora_workspace_bytes(const VilaLlmShape* s, int T, int r);
int vila_llm_prefill_lora(const VilaLlmWeights* w, const VilaLoraLayer* lora /*[n_layers] host*/, int r, float scale, const void* embeds,
                          const int32_t* positions, const int32_t* cu_seqlens, int n_seq, int T, int max_seqlen, const int32_t* seq_of_tok,
                          const VilaKvCache* cache, const int32_t* last_rows, int n_last, float* last_logits, float* all_logits, void* final_hidden,
                          void* workspace, size_t workspace_bytes, vila_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

// Internal launcher declarations shared by the translation units of libvila_hip.so.
#pragma once
#include "common.h"

// stream handle of the C-ABI -> hipStream_t, with the calling thread switched to the stream's device (api.hip)
hipStream_t vila_stream_enter(void* stream);

enum { EPI_NONE = 0, EPI_GELU_TANH = 1, EPI_GELU_ERF = 2, EPI_GATEUP = 3 };

// C[M,N] = epi(A[M,K] . W[N,K]^T + bias[N]) (+ residual[M,N]);  bf16 in, fp32 accumulate, bf16 (or fp32) out.
// EPI_GATEUP: C[M,N] = silu(A.W^T) * (A.W2^T)   (N = intermediate size)
struct GemmArgs {
    const bf16_t* A = nullptr; int64_t lda = 0;
    const bf16_t* W = nullptr; int64_t ldw = 0;
    const bf16_t* W2 = nullptr;
    const bf16_t* bias = nullptr;
    const bf16_t* residual = nullptr; int64_t ldr = 0;
    int res_mod = 0;                            // > 0: the residual has res_mod rows and row m reads residual[m % res_mod] (position embeddings of a batch)
    void* C = nullptr; int64_t ldc = 0; int out_f32 = 0;
    int M = 0, N = 0, K = 0; int epi = EPI_NONE;
    float* ws = nullptr; size_t ws_bytes = 0;   // optional fp32 workspace: enables split-K for under-filled grids
    // operand storage (gemm256_kernel.h): 0 = contraction-contiguous X[rows][K] (forward layout), 1 = contraction-major X[K][rows]
    // (dgrad reads W[N,K] with b_cm; wgrad reads dY[T,N] and X[T,K] with a_cm and b_cm); lda / ldw are the STORED leading dimensions
    int a_cm = 0, b_cm = 0;
    // optional fused follow-up normalisation of the OUTPUT rows (the next block's LayerNorm / RMSNorm): honoured only where the launcher takes
    // the split-K path (its reduce kernel holds whole rows) — then *norm_done = 1 and norm_out[M][N] = norm(C) with C as it was just stored
    const bf16_t* norm_w = nullptr; const bf16_t* norm_b = nullptr; float norm_eps = 0.f; int norm_rms = 0;
    bf16_t* norm_out = nullptr; int* norm_done = nullptr;
    // optional fused follow-up of a q/k/v projection (prefill): bias -> bf16 -> RoPE on the q and k heads -> K / V rows into the cache, i.e. what
    // rope_kv_kernel (elementwise.hip) does to C afterwards.  Honoured only on the split-K path (its reduce then does both) — *rope_done = 1
    const float* rope_cs = nullptr; const float* rope_sn = nullptr; const int32_t* rope_pos = nullptr; const int32_t* rope_seq = nullptr;
    bf16_t* rope_kc = nullptr; bf16_t* rope_vc = nullptr; int rope_nq = 0, rope_nkv = 0, rope_hd = 0, rope_max_ctx = 0; int* rope_done = nullptr;
};
int launch_gemm(const GemmArgs& a, hipStream_t s);
// a complete, applicable RoPE + KV follow-up request (the output row IS the fused q|k|v row, no residual, heads of a multiple of 16)
static inline bool gemm_rope_offer(const GemmArgs& a) {
    return a.rope_done != nullptr && a.rope_cs != nullptr && a.rope_sn != nullptr && a.rope_pos != nullptr && a.rope_hd > 0 && a.rope_hd % 16 == 0 &&
           a.N == (a.rope_nq + 2 * a.rope_nkv) * a.rope_hd && a.residual == nullptr && a.epi == EPI_NONE && !a.out_f32 && a.ldc % 8 == 0;
}

// ---- normalisation / elementwise (elementwise.hip) ----
int launch_layernorm(const bf16_t* x, const bf16_t* w, const bf16_t* b, bf16_t* y, int rows, int cols, float eps, hipStream_t s);
int launch_rmsnorm(const bf16_t* x, const bf16_t* w, bf16_t* y, int rows, int cols, float eps, hipStream_t s);
// im2col for Conv2d(k=s=P, valid): pixels [B,C,H,W] bf16 -> patches [B*gh*gw, Kp] (K = C*P*P zero-padded to Kp)
int launch_im2col(const bf16_t* px, bf16_t* out, int B, int C, int H, int W, int P, int Kp, hipStream_t s);
int launch_pad_rows(const bf16_t* in, bf16_t* out, int rows, int K, int Kp, hipStream_t s);
int launch_add_pos(bf16_t* x, const bf16_t* pos, int B, int N, int D, hipStream_t s);
// space-to-depth (flat_square k x k with zero padding) : x [B, g*g, C] -> y [B, gd*gd, k*k*C]
int launch_space_to_depth(const bf16_t* x, bf16_t* y, int B, int g, int C, int k, hipStream_t s);
// rope table: positions [S] i32 -> cos/sin [S][hd/2] stored as bf16-rounded fp32 (HF casts cos/sin to the act dtype)
int launch_rope_table(const int32_t* pos, float* cs, float* sn, int S, int hd, float theta, hipStream_t s);
// applies bias-added q,k RoPE in place on the fused qkv buffer [S][q+2kv] and scatters k,v into the cache
int launch_rope_kv(bf16_t* qkv, const float* cs, const float* sn, const int32_t* pos, const int32_t* seq_of_tok,
                   bf16_t* kcache, bf16_t* vcache, int S, int nq, int nkv, int hd, int max_ctx, hipStream_t s);
int launch_embed_gather(const bf16_t* table, const int64_t* ids, bf16_t* out, int n, int H, int64_t vocab, hipStream_t s);
int launch_copy_rows(const bf16_t* src, bf16_t* dst, const int32_t* src_row, const int32_t* dst_row, int n, int H, hipStream_t s);
int launch_argmax(const float* logits, int V, int64_t* out, float* tmpv, int* tmpi, hipStream_t s);
// probe of wave_sum_xor (gemv_common.h) against wave_sum: one wave per 64 inputs, every lane writes both sums
int launch_wave_sum_probe(const float* in, float* out_xor, float* out_shfl, int n_waves, hipStream_t s);
// final pick of the batch-1 greedy step: merges the n (max, index) pairs left by the lm_head GEMV (GemvArgs::amax_v), writes *token and advances
// the state like launch_decode_advance
int launch_argmax_pick_advance(const float* tv, const int* ti, int n, int64_t* token, int32_t* pos, int64_t* out_ids, int32_t* n_out, int max_out,
                               hipStream_t s);
// stochastic token choice (sample.hip): temperature -> top-k (1..64) -> top-p -> draw; counter = device scalar mixed into the RNG
size_t sample_workspace_bytes();
int launch_sample(const float* logits, int n, float temperature, int top_k, float top_p, uint64_t seed, const uint64_t* seed_dev, const int32_t* counter, int64_t* out,
                  void* workspace, float* prob_out, hipStream_t s);
// the batched sampler: one choice per row of logits [n][vocab] (n <= 16, top_k 1..64), every per-row parameter a device array [n]; temperature <= 0 =
// greedy row.  out[row] = the token; dist_out (nullable) [n][128]; adv_pos != nullptr: also the batched decode step's state advance
// (out_ids[row][n_out[row]++] = token, pos[row] = counter[row] + 1)
// any_k (opt-in): one launch more draws the rows with top_k = 0 or > 64 by the solo sampler's exact path, in the same workspace; dense_out
// (nullable, any_k only) [n][ld_dense]: such a row's distribution over the vocabulary
struct BatchSampling { const float* temperature; const int32_t* top_k; const float* top_p; const uint64_t* seed; };
size_t sample_batch_workspace_bytes(int n);
int launch_sample_batch(const float* logits, int64_t ld_logits, int n, int vocab, const BatchSampling& sp, int sp_stride, const int32_t* counter, int64_t* out,
                        void* workspace, float* dist_out, int32_t* adv_pos, int64_t* adv_out_ids, int32_t* adv_n_out, int max_out, hipStream_t s,
                        bool any_k = false, float* dense_out = nullptr, int64_t ld_dense = 0);
// ---- the (value, index) keys of sample.hip, shared with logprob.hip (device code; moved here unchanged) ----
#if defined(__HIPCC__)
// order-preserving key: larger float -> larger key; ties broken towards the LOWER index (index stored inverted in the low bits)
__device__ __forceinline__ uint64_t smp_key(float v, int idx) {
    uint32_t u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)u << 32) | (uint32_t)(0x7fffffff - idx);
}
__device__ __forceinline__ float smp_val(uint64_t k) {
    uint32_t u = (uint32_t)(k >> 32);
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __uint_as_float(u);
}
__device__ __forceinline__ int smp_idx(uint64_t k) { return 0x7fffffff - (int)(uint32_t)(k & 0xffffffffu); }
#endif
// repetition / presence / frequency penalties in front of the pick (penalty.hip): logits [n][ld] -> out [n][ld_out], counts[row][token[row]] bumped first
// (token nullable: no bump), every parameter a device array [n]; pick_v / pick_i (nullable) [n][n_slices]: the (max, first index) pair of each slice of
// the processed row — with PEN_PICK_SLICES slices the pairs bdec_pick2_kernel merges
struct Penalties { const float* repetition; const float* presence; const float* frequency; uint16_t* counts; int64_t ld_counts; };
constexpr int PEN_PICK_SLICES = 32;      // = decode_batch.hip's PICK_SLICES
constexpr int PEN_SOLO_SLICES = 256;     // the batch-1 step: one block per CU, merged by launch_argmax_pick_advance
int launch_penalize(const float* logits, int64_t ld, int n, int vocab, const Penalties& p, const int64_t* token, float* out, int64_t ld_out, int n_slices,
                    float* pick_v, int* pick_i, hipStream_t s);
// the verify form: n <= PEN_VERIFY_MAX_ROWS rows of ONE sequence, row i penalised with counts[0][v] + #{j <= i : token[j] == v} (saturating) and entry 0
// of the parameter arrays; the table is only read.  launch_verify_commit, behind the accept, by one thread: counts[consumed[j]] bumped for j = 0 .. *n_accept
// and *state = states[*n_accept] (counts / state nullable, not both)
constexpr int PEN_VERIFY_MAX_ROWS = 16;
int launch_penalize_verify(const float* logits, int64_t ld, int n, int vocab, const Penalties& p, const int64_t* token, float* out, int64_t ld_out, int n_slices,
                           float* pick_v, int* pick_i, hipStream_t s);
int launch_verify_commit(uint16_t* counts, int vocab, int32_t* state, const int64_t* consumed, const int32_t* states, const int32_t* n_accept, int n,
                         hipStream_t s);
// structured output (constrain.hip): a token-class automaton per row behind the penalties and in front of the pick.  state[r] < 0 = unconstrained row;
// token (nullable: no advance) = the token the step consumes; out may alias logits; pick_v / pick_i as launch_penalize's.  Two launches (one without token).
constexpr int CON_MAX_CLASSES = 4096;    // = VILA_CONSTRAIN_MAX_CLASSES: one state's table row in LDS
struct Constraints { int32_t* state; const uint16_t* cls; int64_t ld_cls; const int16_t* next; int64_t ld_next; const int32_t* n_classes; };
int launch_constrain(const float* logits, int64_t ld, int n, int vocab, const Constraints& c, const int64_t* token, float* out, int64_t ld_out, int n_slices,
                     float* pick_v, int* pick_i, hipStream_t s);
// the verify form: launch_verify_chain walks automaton 0 along token[0 .. n - 1] of ONE sequence into states_out (c->state is only read; c NULL: no
// chain) and keeps the tokens in consumed (nullable); launch_constrain_rows masks row i from states[i] with automaton 0's classes and table
int launch_verify_chain(const Constraints* c, const int64_t* token, int n, int vocab, int32_t* states_out, int64_t* consumed, hipStream_t s);
int launch_constrain_rows(const float* logits, int64_t ld, int n, int vocab, const Constraints& c, const int32_t* states, float* out, int64_t ld_out, int n_slices,
                          float* pick_v, int* pick_i, hipStream_t s);
// log-probabilities of the chosen token and of the LP_TOP most likely ones from raw logits [n][ld] (logprob.hip): row r writes record rec[r] + rec_bias
// (rec nullable) of token_lp [n][max_rec] and top_lp / top_id [n][max_rec][LP_TOP] (both or neither); an index outside 0 .. max_rec - 1 writes nothing
constexpr int LP_TOP = 20;
size_t logprob_workspace_bytes(int n);
int logprob_slice_width(int vocab);
int launch_logprobs(const float* logits, int64_t ld, int n, int vocab, const int64_t* token, int top_n, const int32_t* rec, int rec_bias, float* token_lp,
                    float* top_lp, int32_t* top_id, int max_rec, void* workspace, hipStream_t s,
                    bool one_seq = false);                                    // one_seq: every row writes output row 0 (the steps of ONE sequence)
// behind a verify step's accept: tok_rows[i] / rec_rows[i] = the token row i emitted and its record, -1 / -1 for the rows behind *n_accept
int launch_logprobs_verify_index(const int64_t* out_ids, const int32_t* n_out, const int32_t* n_accept, int n, int max_out, int64_t* tok_rows, int32_t* rec_rows,
                                 hipStream_t s);
// dynamic_s2 merge (s2.hip): tower output -> projector input, desc = device [n_blocks][6] {tile_base, bh, bw, i, j, single}
int launch_s2_merge(const bf16_t* feats, bf16_t* out, const int32_t* desc, int n_blocks, int g, int C, int n_scales, const int* splits,
                    hipStream_t s);
// adjoint of the merge: dy [n_blocks][g*g][n_scales*C] -> dx [n_tiles][g*g][C]; tdesc = device [n_tiles][8] {first block of the image,
// bh, bw, scale, tile row, tile col, single, 0}
int launch_s2_merge_bwd(const bf16_t* dy, bf16_t* dx, const int32_t* tdesc, int n_tiles, int g, int C, int n_scales, const int* splits,
                        hipStream_t s);

// video token assembly (video.hip): temporal / spatial mean pooling + start / end token rows per pooled frame
int launch_video_pool(const bf16_t* feats, bf16_t* out, int nt, int nl, int C, int pt, int ph, int pw, const bf16_t* start_rows, int n_start,
                      const bf16_t* end_rows, int n_end, hipStream_t s);
int launch_video_pool_bwd(const bf16_t* dpooled, bf16_t* dfeats, int nt, int nl, int C, int pt, int ph, int pw, int accumulate, hipStream_t s);

// ---- W8A8 (gemm_i8.hip): Y = epi((Xq . Wq^T) * sx[m] * sw[n] + bias) (+ residual), int8 operands, int32 accumulate, bf16 out ----
int launch_gemm_i8(const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw, const float* sx, const float* sw, const bf16_t* bias,
                   const bf16_t* residual, int64_t ldr, bf16_t* C, int64_t ldc, int M, int N, int K, int epi, hipStream_t s);
int launch_quant_rows_i8(const bf16_t* x, int8_t* q, float* scale, int rows, int cols, hipStream_t s);

// ---- attention (attn.hip) ----
struct AttnArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o;
    int64_t q_tok_stride, k_tok_stride, v_tok_stride, o_tok_stride;   // elements between consecutive tokens
    int q_head_stride, k_head_stride, v_head_stride, o_head_stride;  // elements between heads
    const int32_t* cu_seqlens;   // [n_seq+1] device, or null => one sequence of total_tokens
    int n_seq, total_tokens, max_seqlen;
    int n_q_heads, n_kv_heads, head_dim;
    int causal; float scale;
    float* lse;                  // optional [n_q_heads][total_tokens] fp32 (natural-log LSE) for backward
};
int launch_attn_fwd(const AttnArgs& a, hipStream_t s);
// causal attention with a key prefix (append prefill): q [T][ldq] at positions past .. past + T - 1, keys / values = ONE cache slot of one layer
// [kv_heads][max_ctx][128]; row i attends keys 0 .. past + i and nothing at or beyond past + T is read; o [T][ldo]
int launch_attn_append(const bf16_t* q, int64_t ldq, const bf16_t* kslot, const bf16_t* vslot, int past, int T, bf16_t* o, int64_t ldo, int q_heads,
                       int kv_heads, int max_ctx, float scale, hipStream_t s);
// pos[i] = past + i, seq_of_tok[i] = slot for i < T
int launch_append_index(int32_t* pos, int32_t* seq_of_tok, int past, int slot, int T, hipStream_t s);

// ---- decode (gemv.hip; the attention: attn_decode.hip, shared device pieces and constants in attn_decode.h) ----
struct GemvArgs {
    const bf16_t* x;          // [K] activations (bf16)
    const bf16_t* norm_w;     // optional RMSNorm gain fused in front (null = none)
    float eps;
    const bf16_t* W;          // [N][K]
    const bf16_t* W2;         // gate/up mode: up rows
    const bf16_t* bias;       // [N] optional
    const bf16_t* residual;   // [N] optional, added after
    bf16_t* y;                // [N] bf16 out (or null)
    float* y_f32;             // [N] fp32 out (logits) (or null)
    int N, K; int mode;       // 0 plain, 1 gate/up silu-mul, 2 plain with x = merge of the decode-attention partials
    const float* part_o; const float* part_ml; const int32_t* pos_ptr; int n_splits;   // mode 2
    int split_keys;           // mode 2: keys per partial slice (0 = the 64-key slices of attn_decode_partial)
    float* amax_v; int* amax_i;   // mode 0 with y_f32, optional: one (max, index) pair of the fp32 outputs per block, [gemv_grid_blocks(N)]
};
int launch_gemv(const GemvArgs& a, hipStream_t s);
int gemv_grid_blocks(int N);  // blocks of launch_gemv's grid for N rows in modes 0 and 1
struct QkvDecodeArgs {
    const bf16_t* x; const bf16_t* norm_w; float eps;
    const bf16_t* Wqkv; const bf16_t* bqkv;   // fused [q+2kv][K], [q+2kv]
    bf16_t* q_out;                             // [nq*hd]
    bf16_t* kcache; bf16_t* vcache;            // this layer's [nkv][max_ctx][hd]
    const int32_t* pos_ptr;                    // device scalar: position of the new token (= current context length)
    const float* rope_cs;                      // [hd] cos | sin of that position (decode_prologue_kernel)
    int K, nq, nkv, hd, max_ctx;
};
int launch_qkv_decode(const QkvDecodeArgs& a, hipStream_t s);
struct AttnDecodeArgs {
    const bf16_t* q; const bf16_t* kcache; const bf16_t* vcache;
    bf16_t* o;                       // [nq*hd] merged output (second launch); null = partials only
    float* part_o; float* part_ml;   // workspace: [n_splits][nq][hd], [n_splits][nq][2]
    const int32_t* pos_ptr;          // context length BEFORE this token; keys 0..pos inclusive are attended
    int nq, nkv, hd, max_ctx, n_splits; float scale;
    int split256;                    // 1: per-head blocks over 256-key slices, partials only (merged in the o_proj GEMV prologue)
    // row = blockIdx.z reads q + row * q_row_stride, cache slot row (+ row * slot_stride), pos_ptr[row]; the three strides are meaningful only for
    // launch_attn_decode_rows (which fills them) and zero otherwise
    int64_t q_row_stride, o_row_stride, slot_stride;
};
int launch_attn_decode(const AttnDecodeArgs& a, hipStream_t s);
int launch_attn_decode_rows(const AttnDecodeArgs& a, int n_rows, int64_t q_row_stride, int64_t o_row_stride, int64_t slot_stride, hipStream_t s);
// batched decode step (decode_batch.hip)
struct BDecodeArgs {
    const void* embed; const void* norm_w; const void* lm_head;
    int hidden, inter, n_layers, q_heads, kv_heads, head_dim, vocab; float rms_eps, rope_theta;
};
struct BLayer { const void *ln1_w, *wqkv, *bqkv, *wo, *ln2_w, *w_gate, *w_up, *w_down; };
// the int4 projections of a layer (quant.py W4Weights, layout gemv_w4.hip); with them the step runs the four projections as W4A16 batched
// GEMVs (gemv_w4_batch.hip) and reads no bf16 projection pointer of BLayer (bqkv, the fused q|k|v bias, is still read)
struct BLayerW4 { const void *qkv_q, *qkv_sz, *o_q, *o_sz, *gateup_q, *gateup_sz, *down_q, *down_sz; };
// attention of the batched step: up to BDEC_SHORT_CTX positions one slice per 256-key chunk of the capacity; beyond, blocks walk chunks s, s + nsl, ...
// with nsl = min(chunks of the capacity, BDEC_SLICE_CAP).  BDEC_MAX_SLICES bounds what the test hook may force (and sizes the long workspace).
#define BDEC_SHORT_CTX 2048
#define BDEC_MAX_CTX 32768        // Qwen2.5's max_position_embeddings
#define BDEC_SLICE_CAP 8          // measured against 16 and 32 (profiles/long_batch_decode_bench.json): best at n = 8 and 16, within 1 - 4 % at n = 2
#define BDEC_MAX_SLICES 32
size_t bdecode_workspace_bytes(int H, int F, int QS, int hd, int n, int max_ctx = BDEC_SHORT_CTX);   // the same bytes for every max_ctx <= 2048
// the batched step's attention (attn_decode.hip).  The form at a capacity: the short one with a slice per chunk, or the walking one with nsl slices
struct BAttnForm { bool walk; int nsl; };
BAttnForm bdec_attn_form(int max_ctx);
bool bdec_group_ok(int G);              // GQA group sizes the two forms are instantiated for
int bdec_ws_slices(int max_ctx);        // partial slots per (row, query head) that a workspace holds at this capacity
// the launches of one layer on partials laid out for f.nsl slices; returns 1, with nothing launched, when the short form has no instantiation for the
// GQA group (the caller then runs launch_attn_decode_rows)
int bdecode_attn_launch(const BAttnForm& f, const bf16_t* q, int64_t ldq, const bf16_t* kcache, const bf16_t* vcache, int64_t slot_stride, const int32_t* pos,
                        bf16_t* o, int64_t ldo, int rows, int nq, int nkv, int max_ctx, float scale, float* part_o, float* part_ml, hipStream_t s);
void bdecode_force_slices(int nsl);
int bdecode_attn_slices(int max_ctx);   // slices of the walking form at this capacity under the current hook, 0 = the short form
// the step's attention on its own: q [rows][ldq], o [rows][ldo], one layer's cache [slots][nkv][max_ctx][128], keys 0 .. pos[row] of slot `row`
size_t bdecode_attn_workspace_bytes(int rows, int nq, int max_ctx);
int bdecode_attn(const bf16_t* q, int64_t ldq, const bf16_t* kcache, const bf16_t* vcache, int64_t slot_stride, const int32_t* pos, bf16_t* o, int64_t ldo,
                 int rows, int nq, int nkv, int max_ctx, float scale, void* workspace, size_t workspace_bytes, hipStream_t s);
// a session whose rows share a prompt prefix (attn_decode.hip, behind the verify form): slot `prefix_slot` of the cache holds keys 0 .. *shared_len - 1 (a
// multiple of 256) of every row with uses[row] != 0, which reads its own slot from there on; other rows are ordinary.  Three launches per layer.
struct BPrefix { int prefix_slot; const int32_t* shared_len; const int32_t* uses; };
size_t bprefix_attn_workspace_bytes(int rows, int nq, int max_ctx);
int bprefix_attn_launch(const bf16_t* q, int64_t ldq, const bf16_t* kcache, const bf16_t* vcache, int64_t slot_stride, int prefix_slot, const int32_t* shared_len,
                        const int32_t* uses, const int32_t* pos, bf16_t* o, int64_t ldo, int rows, int nq, int nkv, int max_ctx, float scale, float* part_o,
                        float* part_ml, float* pfx_o, float* pfx_ml, hipStream_t s);
int bprefix_attn(const bf16_t* q, int64_t ldq, const bf16_t* kcache, const bf16_t* vcache, int64_t slot_stride, int n_slots, int prefix_slot,
                 const int32_t* shared_len, int shared_len_host, const int32_t* uses, const int32_t* pos, bf16_t* o, int64_t ldo, int rows, int nq, int nkv,
                 int max_ctx, float scale, void* workspace, size_t workspace_bytes, hipStream_t s);
// per-row LoRA adapters in the batched step (lora_decode.hip): row i runs under slot row_adapter[i] of a bank of `capacity` adapters of rank r, or under
// none (-1).  Per layer and stack, A [capacity][Rs][K] bf16 (Rs = 3 r: q|k|v, 2 r: gate|up, r: o, down) and B packed [capacity][r / 8][N][8] bf16 over the
// stack's N output columns; scale [capacity] fp32.  T [16][3 r] and D [16][max(q + 2 kv, 2 inter)] fp32 are the step's scratch.
#define LORA_MAX_SLOTS 32
struct BLoraLayer { const void *a_qkv, *b_qkv, *a_o, *b_o, *a_gateup, *b_gateup, *a_down, *b_down; };
struct BLora { const BLoraLayer* layers; const float* scale; const int32_t* row_adapter; int capacity, r; float* T; float* D; };
int launch_lora_shrink(const bf16_t* x, int64_t ldx, int n, const bf16_t* A, int64_t slot_stride, const float* scale, const int32_t* row_adapter, int capacity,
                       float* T, int64_t ldt, int Rs, int K, hipStream_t s);
int launch_lora_expand(const float* T, int64_t ldt, int n, const bf16_t* B, int64_t slot_stride, const int32_t* row_adapter, int capacity, float* D, int64_t ldd,
                       int N, int r, int c1, int c2, hipStream_t s);
// prefix != nullptr: the step of such a session (n_slots counts the prefix slot; the workspace is bdecode_prefix_workspace_bytes)
size_t bdecode_prefix_workspace_bytes(int H, int F, int QS, int hd, int n, int max_ctx);
int bdecode_step(const BDecodeArgs& m, const BLayer* layers, bf16_t* kcache, bf16_t* vcache, int max_ctx, int n_slots, int n, int32_t* pos, int64_t* token,
                 int64_t* out_ids, int32_t* n_out, int max_out, float* logits, void* workspace, size_t workspace_bytes, hipStream_t s,
                 const BLayerW4* qlayers = nullptr, const BatchSampling* sampling = nullptr, void* sampling_ws = nullptr, const BPrefix* prefix = nullptr,
                 const Penalties* pen = nullptr, float* pen_out = nullptr,    // pen: the pick runs on the penalised rows, written to pen_out [n][vocab]
                 const Constraints* con = nullptr,                            // con: ... masked by the rows' automata (behind the penalties), in pen_out as well
                 bool any_k = false,                                          // any_k: the sampled pick serves every top_k >= 0 (launch_sample_batch)
                 const BLora* lora = nullptr);                                // lora: every row under its own adapter of the bank (bf16 layers, no prefix)
// the verify step (greedy speculative decoding): n rows = n consecutive positions of ONE sequence in ONE slot.  Its attention (attn_decode.hip
// bdec_attn_shared_kernel) reads the slot's K/V once for all rows; `pos` is the device scalar of the state, row i sees keys 0 .. min(pos + i, max_ctx - 1)
int bverify_attn_slices(int max_ctx);
size_t bverify_attn_workspace_bytes(int n, int nq, int max_ctx);
int bverify_attn_launch(const bf16_t* q, int64_t ldq, const bf16_t* kslot, const bf16_t* vslot, const int32_t* pos, bf16_t* o, int64_t ldo, int n, int nq,
                        int nkv, int max_ctx, float scale, float* part_o, float* part_ml, hipStream_t s);
int bverify_attn(const bf16_t* q, int64_t ldq, const bf16_t* kslot, const bf16_t* vslot, const int32_t* pos, bf16_t* o, int64_t ldo, int n, int nq, int nkv,
                 int max_ctx, float scale, void* workspace, size_t workspace_bytes, hipStream_t s);
// the device state of a verify session (include/vila_hip.h VilaDecodeVerify) and the step: draft -> forward of n rows -> accept
struct BVerifyState {
    int n, slot;
    int32_t* pos; int64_t* token; int32_t* n_draft; int64_t* out_ids; int32_t* n_out; int max_out; float* logits; int32_t* n_accept;
    int64_t* hist; int32_t* n_hist; int hist_cap, max_ngram;
    const int64_t* cand; const int32_t* n_cand;
};
// sampling != nullptr: the sampled verify step — row i's a[i] is drawn by the batched sampler with counter pos + i from ONE-entry parameter arrays
// (every row reads entry 0); the workspace is then bverify_sample_workspace_bytes
size_t bverify_workspace_bytes(int H, int F, int QS, int hd, int n, int max_ctx);
size_t bverify_sample_workspace_bytes(int H, int F, int QS, int hd, int n, int max_ctx);
// the processing chain of a verify step (all nullable): penalties and an automaton of ONE sequence in front of the pick / draw, committed behind the
// accept, and the records of the accepted rows.  With one of them the workspace is bverify_processed_workspace_bytes, whatever `sampling`.
struct BVerifyProc {
    const Penalties* pen; const Constraints* con;
    float* lp_tok; float* lp_top; int32_t* lp_id; int lp_max_rec;             // lp_tok NULL: no records; lp_top / lp_id both or neither
};
size_t bverify_processed_workspace_bytes(int H, int F, int QS, int hd, int n, int max_ctx, int vocab);
int bverify_step(const BDecodeArgs& m, const BLayer* layers, bf16_t* kcache, bf16_t* vcache, int max_ctx, int n_slots, const BVerifyState& st, void* workspace,
                 size_t workspace_bytes, hipStream_t s, const BLayerW4* qlayers = nullptr, const BatchSampling* sampling = nullptr,
                 bool any_k = false,                                          // any_k: the rows' draws serve every top_k >= 0
                 const BVerifyProc* proc = nullptr);
int launch_verify_draft(const int64_t* hist, const int32_t* n_hist, int max_ngram, const int64_t* cand, const int32_t* n_cand, const int32_t* n_out, int n,
                        int64_t* token, int32_t* n_draft, const int32_t* pos, int32_t* pos_rows, hipStream_t s);
int launch_decode_prologue(const bf16_t* table, const int64_t* tok, bf16_t* out, int H, int64_t vocab, const int32_t* pos, float* rope_cs,
                           int hd, float theta, hipStream_t s);
int launch_decode_advance(int32_t* pos, const int64_t* tok, int64_t* out_ids, int32_t* n_out, int max_out, hipStream_t s);

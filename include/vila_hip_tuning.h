/* vila_hip_tuning.h — tuning and test switches of libvila_hip.so.  NOT part of the drop-in boundary (include/vila_hip.h):
 * these are PROCESS-GLOBAL, not thread-safe, and exist for the A/B measurements under tools/ and for the parity tests that pin one
 * kernel variant (tests/test_gpu_ops.py).  A product binding never calls them; every switch defaults to the measured-best policy.
 * Environment equivalents read once at first use: VILA_GEMM_EX, VILA_ATTN_FWD=v1, VILA_ATTN_KS, VILA_ATTN_BWD=v1, VILA_DECODE_ATTN. */
#ifndef VILA_HIP_TUNING_H
#define VILA_HIP_TUNING_H
#ifdef __cplusplus
extern "C" {
#endif
/* tuning hook for the 256x256 kernel's K-loop schedule (gemm256_kernel.h SCHED): 0 = each layout's default, 1 / 2 / 3 / 5 / 6 = that schedule,
 * 9 = ablation without DMA (timing only), 10 = the round-1 schedule (SCHED 0) */
void vila_gemm_force_sched(int sched);
/* tuning hook for the launch policy fed by a workspace: whole rounds of 256x256 tiles + K-sliced tail tiles (1 = on, default; 0 = off) */
void vila_gemm_force_hybrid(int on);
/* tuning hook for the decode step's attention (caches up to 2048 positions): 2 (default) / 1 = per-head blocks over 256-key slices with the
 * merge in the o_proj GEMV's prologue (512 / 256 o_proj blocks), 0 = one block per query head over the whole context + plain o_proj */
void vila_decode_force_attn(int mode);
/* tuning hook: output rows per tile of the 256-wide kernel: 0 = automatic (192 when it saves tile-times), 192, 256 */
void vila_gemm_force_bm(int bm);
/* tuning / test hook: 0 = automatic tile choice, 1 = 128x128, 2 = 128x64, 3 = 256x128, 4 = 256x256 LDS-DMA, 5 = split-K if possible,
 * 6 / 7 = 128x64 LDS-DMA ring with 4 / 3 stages, 8 = 128x128 ring with 2 stages, 11 = the K-sliced 128x64 ring of gemm_ring_splitk.hip when a
 * workspace is given (automatic for M < 512 since round 5; environment: VILA_RING_SPLITK=0 turns that off), 12 / 13 / 14 = rings 7 / 8 / 6 with the
 * PIPE 2 fragment schedule (inline-asm fragment reads retired by register-tied waits: the ks = 1 reads land under the ks = 0 MFMAs; the default for
 * every ring launch since round 5, environment: VILA_RING_PIPE=0 = plain), 15 / 16 / 17 = the same three rings with the plain schedule */
void vila_gemm_force_tile(int tile);
/* leftover rows (M = 256 k + r, 1 <= r <= 16) as an extra fragment of the last 256-row tile (gemm256_kernel.h, EX): -1 = VILA_GEMM_EX from the
 * environment (default 1), 0 = off, 1 = when it saves a round of tiles (and in every K-sliced launch), 2 = whenever the rows fit (tests) */
void vila_gemm_force_ex(int mode);
/* tile order of the 256-wide kernel (gemm256_kernel.h gemm256_tile_of): -1 = automatic (columns grouped by 4 when the grid has more than 16
 * row tiles), 0 = row-tile-fastest everywhere (rounds 1-2), n > 1 = groups of n columns */
void vila_gemm_force_group(int grp);
/* the K-sliced GEMMs' reduce takes the next block's LayerNorm / RMSNorm along (prefill down_proj -> next input_layernorm, tower fc2 -> next
 * layer_norm1): 1 = on (default), 0 = separate norm launches (A/B and the parity test of the fused kernel); environment: VILA_FUSE_NORM */
void vila_gemm_force_fuse_norm(int on);
/* the launch plan of a bf16 GEMM under the current hooks, as one line of text ("family=... splits=... per=... full=... tail=... ex=... bm=... group=...
 * sched=... ring=... pipe=... reduce=..."; csrc/gemm_plan.h has the fields).  Host only: launches nothing and asks the runtime for no device, so it works
 * without a GPU.  ws_bytes = size of the fp32 workspace (0 = none given); offers: bit 0 = the next block's normalisation, bit 1 = the q/k/v RoPE + KV
 * follow-up (what the prefill offers).  Returns the length written, -1 when buf_len is too small */
int vila_gemm_plan_describe(int M, int N, int K, int epi, int out_f32, int a_cm, int b_cm, size_t ws_bytes, int offers, char* buf, int buf_len);
/* LayerNorm / RMSNorm over rows wider than 1536 columns: every load (x, w, b) requested up front instead of x -> reduce -> w (elementwise.hip
 * norm_block_lat_kernel; bit-identical outputs; on by default since round 5): -1 = VILA_NORM_LAT from the environment (default 1), 0 = off, 1 = on */
void vila_norm_force_lat(int on);
/* prefill (round 6): q/k/v projection K-sliced with bias + RoPE + KV-cache scatter in its reduce (instead of ring GEMM + rope_kv_kernel), and o_proj
 * K-sliced with the post-attention RMSNorm in its reduce (instead of ring GEMM + norm launch); both only where the grid is K-sliced at all
 * (>= 512 rows).  -1 = the environment's choice (VILA_PREFILL_QKV_SPLITK / VILA_PREFILL_OPROJ_SPLITK, default on), 0 = off, 1 = on */
void vila_prefill_force_fusions(int qkv_rope, int oproj_norm);
/* test hook of the attention forward (attn.hip): 0 = automatic (the policy below plus VILA_ATTN_FWD / VILA_ATTN_KS), or one form whatever the grid:
 * 1 = A (256-row blocks, 32 rows per wave), 2 = B (64-row blocks, keys split two ways inside the block), 3 = C (128-row blocks, keys split two ways),
 * 4 = D (128-row blocks, 16 rows per wave), 5 = the round-2 kernel (VILA_ATTN_FWD=v1).  Every form serves head dims 64, 72 and 128 */
void vila_attn_force_fwd(int form);
/* the form (1..5 as above) the automatic policy launches for this grid on the current device; host only, launches nothing */
int vila_attn_fwd_form(int n_seq, int max_seqlen, int n_q_heads);
/* test hook of the append prefill's attention (vila_attn_append_bf16, vila_llm_prefill_append): 0 = automatic (the forward's policy for one sequence
 * of T rows), 1..4 = forms A..D as above whatever the grid (the round-2 kernel has no key-prefix mode) */
void vila_attn_force_append(int form);
/* the form (1..4) the automatic policy launches for an append of T rows on the current device; host only, launches nothing */
int vila_attn_append_form(int T, int n_q_heads);
/* test hook of the attention backward's dQ and dK / dV passes: 0 = VILA_ATTN_BWD from the environment (default: DMA), 1 = the round-1/2 kernels
 * of attn_bwd.hip (VILA_ATTN_BWD=v1), 2 = the DMA-ring kernels of attn_bwd_dma.hip */
void vila_attn_force_bwd(int impl);
/* test / measurement hook of the batched decode step's attention (attn_decode.hip): 0 = automatic (up to 2048 cached positions one slice per
 * 256-key chunk; beyond, blocks that walk chunks s, s + nsl, ... with nsl = min(chunks of the capacity, 8)), n > 0 = the walking form with
 * min(n, 32, chunks of the capacity) slices at ANY capacity, so that a small cache makes blocks walk many chunks */
void vila_decode_batch_force_slices(int nsl);
/* what a step enqueued now would launch for a cache of max_ctx positions: the slice count of the walking form, 0 = the short form; host only */
int vila_decode_batch_slices(int max_ctx);
#ifdef __cplusplus
}
#endif
#endif

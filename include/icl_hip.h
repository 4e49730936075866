/*
 * icl_hip.h — C-ABI of libicl_hip.so, the MI355X (gfx950 / CDNA4) kernel library behind the
 * ICL forward/generate hot path of iiscleap/ICL-speech-text-LLM.
 *
 * The reference has NO FFI of its own: every kernel it runs is reached through PyTorch /
 * transformers / the external SALMONN package.  Each entry point
 * below therefore cites the reference call site (file:line under /root/reference) whose
 * arithmetic it replaces, plus the implicit-op row of SURVEY.md §2.3 (K1..K14).
 *
 * Conventions:
 *   - plain pointers and sizes only; no torch types; every pointer is a DEVICE pointer unless
 *     its name ends in _host;
 *   - no allocation or ownership inside the library: the caller (PyTorch-ROCm on the host
 *     side) allocates inputs, outputs and workspaces;
 *   - every call is asynchronous w.r.t. the host and ordered on `stream` (a hipStream_t passed
 *     as void*); nothing here synchronises, allocates or memcpy's, so every call may be
 *     captured into a hipGraph;
 *   - return value: 0 on success, a negative ICL_E* code otherwise; icl_last_error() returns
 *     a thread-local, human-readable message for the most recent failure on this thread.
 *     A failure never aborts the process and never leaves a kernel running: arguments are
 *     validated on the host before any launch (reference behaviour to preserve: the per-batch
 *     try/except in inference/inference.py:370-373 must be able to continue).
 *   - "bf16" tensors are raw uint16 bit patterns of bfloat16; "f32" is IEEE binary32.
 *   - all matrices are row-major with an explicit leading dimension (in ELEMENTS).
 */
#ifndef ICL_HIP_H
#define ICL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICL_ABI_VERSION 6

/* error codes */
#define ICL_OK 0
#define ICL_EINVAL (-1)  /* bad argument / unsupported shape (message in icl_last_error) */
#define ICL_ELAUNCH (-2) /* hipLaunch / runtime error (message carries hipGetErrorString) */

/* element types for outputs / residuals */
#define ICL_BF16 0
#define ICL_F32 1

/* ---- library ------------------------------------------------------------------------- */
int icl_abi_version(void);
const char* icl_last_error(void);
/* Number of compute units of the current device (used by callers to size split-K). */
int icl_device_cu_count(void);

/* ---- K2/K3/K5/K7/K8/K10/K13/K14: bf16 MFMA GEMM ----------------------------------------
 * C[b][m][n] = epilogue( sum_k A[b][m][k] * W[n][k] )       (W is the PyTorch nn.Linear
 * layout [N,K], K contiguous), fp32 accumulation on v_mfma_f32_16x16x32_bf16.
 * Replaces every nn.Linear / Conv1d-as-GEMM of the path: HF WhisperEncoder / LlamaForCausalLM
 * reached from models/custom_salmon.py:550-554 (encode_speech) and :630-636 / :704-720
 * (llama_model forward / generate).
 *
 * epilogue (applied in this order):  v = acc; v += bias[n] (ICL_EPI_BIAS);
 *   v = gelu_erf(v) (ICL_EPI_GELU);  v = silu(v_gate)*v_up (ICL_EPI_SWIGLU, see below);
 *   v += R[b][m][n] (ICL_EPI_RESIDUAL, R is f32 or bf16 per res_dtype); store as out_dtype.
 * ICL_EPI_SWIGLU: W holds gate/up rows interleaved in blocks of 16 ([g0..g15,u0..u15,g16..]),
 *   N counts the interleaved rows; the output has N/2 columns (ldc refers to that matrix).
 * batch: independent problems on grid.z with element strides (stride 0 = broadcast; W has
 *   no batch stride — the weight is shared).
 * split_k > 1 (only with batch == 1): partial sums go to `workspace` (f32, at least
 *   split_k*M*N elements) and a second kernel reduces them and applies the epilogue.
 * Requirements: K % 64 == 0, lda/ldw % 8 == 0, A/W 16-byte aligned, N % 32 == 0 for SWIGLU.
 */
#define ICL_EPI_BIAS 1
#define ICL_EPI_GELU 2
#define ICL_EPI_RESIDUAL 4
#define ICL_EPI_SWIGLU 8

typedef struct icl_gemm_args {
  const void* A;        /* bf16 [batch][M][lda]            */
  const void* W;        /* bf16 [N][ldw]                   */
  void* C;              /* out_dtype [batch][M][ldc]       */
  const float* bias;    /* f32 [N] or NULL                 */
  const void* R;        /* res_dtype [batch][M][ldr] or NULL */
  float* workspace;     /* f32 split-K partials or NULL    */
  int64_t lda, ldw, ldc, ldr;
  int64_t strideA, strideC, strideR; /* batch strides in elements */
  int32_t M, N, K;
  int32_t batch;
  int32_t epilogue;     /* OR of ICL_EPI_*                 */
  int32_t out_dtype;    /* ICL_BF16 | ICL_F32              */
  int32_t res_dtype;    /* ICL_BF16 | ICL_F32              */
  int32_t split_k;      /* >= 1                            */
  int32_t tile;         /* 0 = auto, 1 = 128x128, 2 = 64x64 (+ split_k), 3 = 256x256 (+ split_k), 4 = decode
                           skinny kernel (M <= 64, batch 1: weights streamed HBM->VGPR, in-block split-K),
                           5 = decode tile for M <= 128 (batch 1, + split_k; 64-row blocks when M <= 64): W must
                           be the decode-packed copy made by icl_pack_decode_weights (ldw is ignored),
                           6 = the skinny kernel (as 4) on the decode-packed copy                       */
} icl_gemm_args;

int icl_gemm_bf16(const icl_gemm_args* args, void* stream);
/* The decode form of "projection back into the residual stream, then the next RMSNorm" (HF LlamaDecoderLayer:
 * hidden = residual + o_proj(attn) ; post_attention_layernorm(hidden) — and down_proj followed by the next layer's
 * input_layernorm / the final norm; reached from models/custom_salmon.py:704-720 through generate): C = R + A W^T in f32
 * (epilogue must be 0 or ICL_EPI_RESIDUAL with an f32 residual, batch 1, f32 output) AND xn[m][:N] = bf16(rmsnorm(C[m]) * gamma).
 * With split_k > 1 the partial slabs are reduced, the residual added, the row stored and normalised by ONE kernel (a launch
 * and a re-read of the row less than icl_gemm_bf16 + icl_rmsnorm; C is bit-identical to that pair, xn sums its squares in a
 * different — fixed — order).  With split_k == 1 (and always on the skinny tiles 4 / 6, which split K inside the block) C is
 * bit-identical to icl_gemm_bf16 with the same arguments, -0.0 included; xn is icl_rmsnorm's when M > 64 or ldc != N, and for
 * M <= 64 with ldc == N it comes from the row-per-block kernel of the split-K path run over C, whose four-wave order of the
 * sum of squares differs from icl_rmsnorm's (xn within 1 bf16 ulp of icl_rmsnorm of C, not bit-identical).  tile 3 accepts
 * split_k > 1 since ABI 5 (K / split_k >= 128).  No reference counterpart (fusion). */
int icl_gemm_rmsnorm_bf16(const icl_gemm_args* args, const float* gamma, float eps, void* xn, int64_t ld_xn, void* stream);
/* Decode-packed copy of a weight matrix for tile 5: row-major bf16 W [N][ldw] -> out, (ceil(N/16)*16) x K bf16
 * elements: per 16-row block a K-long stream of 1-KB pieces (one per 32-wide k-step) in MFMA operand order, so that the
 * decode kernel's wave-loads are 1 KB contiguous (rows >= N are zero).  A layout copy made once at load time (the
 * prefill kernels keep reading the row-major original: HBM is sized for both); no reference counterpart. */
int icl_pack_decode_weights(const void* W, int64_t ldw, int32_t N, int32_t K, void* out, void* stream);
/* ---- K11 (opt-in FP8 weight mode): fp8-weight decode GEMM ---------------------------------
 * The decoder's GEMM weights replaced by their FP8 rounding W' = q * 2^e_n (row n): e_n is the smallest integer with
 * max_k |W[n][k]| <= 448 * 2^e_n (0 for an all-zero row), q[n][k] = W[n][k] / 2^e_n rounded to nearest even in OCP e4m3fn (exact
 * division, never saturated).  W' is exactly representable in bf16.  An MI355X-native option, not a restatement: the reference
 * loads its Llama in 8 bits (bitsandbytes LLM.int8, low_resource=True: inference/inference.py:151, models/custom_salmon.py:49,82)
 * for its batch-1 CLI runs; this mode has its own, exactly defined numerics above.
 *
 * icl_pack_fp8_weights: row-major bf16 W [N][ldw] -> q (ceil(N/16)*16 * K bytes, fp8 decode-packed: per 16-row block a K-long
 * stream of 1-KB pieces, piece (block, k-pair j, lane = fq*16 + fr) = q[16*block + fr][64j + 8fq .. +8] ++ q[..][64j + 32 + 8fq .. +8];
 * rows >= N are zero), scales f32 [N] = 2^e_n, and W' written as bf16 into w_deq [N][ld_deq] (w_deq == W with ld_deq == ldw
 * rewrites W in place).  K % 64 == 0; W, q, w_deq 16-byte aligned.  A load-time call and the one exception to "nothing
 * synchronises": it waits for its stream to return ICL_EINVAL when W holds a NaN or an infinity (q / w_deq are then undefined).
 *
 * icl_gemm_fp8w / icl_gemm_rmsnorm_fp8w: icl_gemm_bf16 / icl_gemm_rmsnorm_bf16 with args->W = the q of icl_pack_fp8_weights
 * (ldw and tile are ignored) and w_scale = its scales, for M <= 64, batch 1.  The skinny decode kernel (tile 6's block shape,
 * per-wave K split, MFMA order and wave-ordered combine) rebuilds W' in registers (fp8 -> f32 -> * 2^e_n -> bf16, all exact) and
 * returns the same bits as tile 6 on the decode-packed copy of W' — every epilogue (bias, SwiGLU, residual) and the RMSNorm
 * pairing included — while reading half the weight bytes.  No reference counterpart (the reference's 8-bit layers are
 * bitsandbytes matmuls behind HF LlamaForCausalLM, reached from models/custom_salmon.py:704-720). */
int icl_pack_fp8_weights(const void* W, int64_t ldw, int32_t N, int32_t K, void* q, float* scales, void* w_deq, int64_t ld_deq,
                         void* stream);
int icl_gemm_fp8w(const icl_gemm_args* args, const float* w_scale, void* stream);
int icl_gemm_rmsnorm_fp8w(const icl_gemm_args* args, const float* w_scale, const float* gamma, float eps, void* xn, int64_t ld_xn,
                          void* stream);
/* The tile id (1|2|3) that tile == 0 resolves to for this problem (pure host function). */
int icl_gemm_select_tile(int32_t M, int32_t N, int32_t K, int32_t batch, int32_t split_k);

/* ---- K3/K5/K10/K13/K14: fused (flash-style) attention forward ---------------------------
 * O[t][h][:] = softmax_j( scale * Q[t][h]·K[j][h] + bias ) · V[j][h]   per packed sequence.
 * Replaces the SDPA inside HF WhisperEncoderLayer / LlamaDecoderLayer / the BEATs
 * MultiheadAttention (reached from models/custom_salmon.py:550-554 and :630-636/:704-720).
 * Sequences are packed back to back: sequence s owns rows cu_seqlens[s] .. cu_seqlens[s+1]-1
 * of Q, K, V and O (queries and keys share the packing: self-attention).
 *   causal != 0   : key j visible to query i iff j <= i (positions relative to the sequence).
 *   kv_lens       : optional int32 [n_seqs]; keys >= kv_lens[s] are masked (BEATs key padding
 *                   mask; queries still run over the whole sequence).  Must be >= 1.
 *   rel_bias      : optional f32 [n_heads][2*rel_span-1] table and rel_gate f32
 *                   [total_rows][n_heads]: bias(i,j,h) = rel_gate[i][h] *
 *                   rel_bias[h][clamp(j-i, -(rel_span-1), rel_span-1) + rel_span-1]
 *                   (BEATs gated relative position bias, K5).
 * head_dim must be 64 or 128.  Q/K/V row strides are in elements (so a fused QKV buffer can
 * be addressed in place); head h lives at column h*head_dim of its row.
 * Contracts the tests rely on (tests/test_gpu_attention_exact.py):
 *   - max_seqlen must bound every sequence length (the grid is sized from it: queries at positions
 *     >= max_seqlen would not be computed).
 *   - An empty sequence (cu_seqlens[s+1] == cu_seqlens[s]) is allowed anywhere in a pack: it owns no
 *     row and its kv_lens entry is not read.
 *   - With kv_lens, the K and V rows in [kv_lens[s], len) must hold FINITE values.  They are staged
 *     with their 64-key tile; their scores are replaced (any finite K gives the same bits as zeros) and
 *     their weight is exactly 0, but 0 * NaN or 0 * Inf in the PV product is NaN.  Rows past len (cache
 *     layout: up to max_len) are never read and may hold anything.
 */
typedef struct icl_attn_args {
  const void* Q; const void* K; const void* V; /* bf16 */
  void* O;                                     /* bf16 [total_rows][ldo] */
  const int32_t* cu_seqlens;                   /* int32 [n_seqs+1] (device) */
  const int32_t* kv_lens;                      /* int32 [n_seqs] or NULL (device) */
  const float* rel_bias;                       /* f32 [n_heads][2*rel_span-1] or NULL */
  const float* rel_gate;                       /* f32 [total_rows][n_heads] or NULL */
  int64_t ldq, ldk, ldv, ldo;
  int32_t n_seqs, max_seqlen, n_heads, head_dim;
  int32_t causal, rel_span;
  float scale;
  int32_t n_kv_heads;                          /* grouped-query attention: K/V heads (0 = n_heads).  Must divide n_heads and
                                                  may differ from it only at head_dim 128; query head h reads K/V head
                                                  h / (n_heads / n_kv_heads): column block (h / G)*head_dim of packed K/V
                                                  rows, or (h / G)*kv_head_stride in a cache whose kv_seq_stride describes
                                                  n_kv_heads heads.  Same kernel and arithmetic as the launch with
                                                  n_kv_heads = 0 on K/V expanded per group: bit-identical output            */
  int64_t kv_seq_stride, kv_head_stride;       /* both 0: K/V rows are packed like Q (row cu_seqlens[s] + j, head h at
                                                  column h*head_dim, row strides ldk / ldv).  Both > 0: K/V are read from a
                                                  cache, key j of (sequence s, head h) at K + s*kv_seq_stride +
                                                  h*kv_head_stride + j*ldk (elements) — the Llama prefill reads back what
                                                  the fused QKV epilogue appended: [n_seqs][n_heads][max_len][head_dim],
                                                  ldk = ldv = head_dim                                              */
} icl_attn_args;

int icl_attn_fwd_bf16(const icl_attn_args* args, void* stream);

/* The suffix-query form of icl_attn_fwd_bf16 (head_dim 128, causal, no bias, no kv_lens): sequence s attends with only its LAST
 * q_len(s) = cu_q[s+1] - cu_q[s] queries, 0 <= q_len(s) <= kv_len(s) = cu_seqlens[s+1] - cu_seqlens[s].  Q and O are packed by
 * cu_q (int32 [n_seqs+1], device): query i of sequence s is row cu_q[s] + i and sits at position kv_len(s) - q_len(s) + i.
 * K / V are addressed by cu_seqlens as in icl_attn_fwd_bf16 (packed rows, or the cache layout); max_seqlen bounds kv_len.
 * Every query runs in the wave, lane and K/V tile sequence it has in the full launch: O rows are bit-identical to the rows
 * icl_attn_fwd_bf16 writes at the same positions.  The last decoder layer of a prefill uses it with q_len = 1.
 */
int icl_attn_fwd_suffix_bf16(const icl_attn_args* args, const int32_t* cu_q, void* stream);

/* ---- K11: single-token decode attention over the KV cache --------------------------------
 * One new query per sequence against cache rows [0, lens[b]) (the new token's K/V must
 * already be in the cache).  Cache layout: [n_seqs][n_heads][max_len][head_dim] bf16.
 * Replaces the cached-key SDPA inside HF GenerationMixin's greedy loop,
 * models/custom_salmon.py:704-720.
 */
int icl_attn_decode_bf16(const void* Q, int64_t ldq, const void* Kc, const void* Vc, void* O,
                         int64_t ldo, const int32_t* lens, int32_t n_seqs, int32_t n_heads,
                         int32_t head_dim, int32_t max_len, float scale, void* stream);

/* ---- K11: grouped-query decode attention ---------------------------------------------------------
 * icl_attn_decode_bf16 for a decoder whose G = n_heads / n_kv_heads query heads share one K/V head (2 <= G <= 8, head_dim
 * 128; G = 1 runs icl_attn_decode_bf16).  Q / O hold n_heads heads per row, the cache n_kv_heads:
 * [n_seqs][n_kv_heads][max_len][head_dim] bf16; query head h attends over K/V head h / G.  One workgroup per (sequence,
 * K/V head) loads every cache row ONCE and uses it for its G query heads, so a launch reads 1/G of the bytes
 * icl_attn_decode_bf16 reads from the per-group expanded cache.  Every query head folds the keys of icl_attn_decode_bf16's
 * streams in their order: the output is that call's on the expanded cache up to the compiler's FMA contraction.
 * Replaces repeat_kv + the cached-key SDPA of transformers' LlamaAttention in a decode step.
 */
int icl_attn_decode_gqa_bf16(const void* Q, int64_t ldq, const void* Kc, const void* Vc, void* O, int64_t ldo,
                             const int32_t* lens, int32_t n_seqs, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim,
                             int32_t max_len, float scale, void* stream);

/* ---- prompt-attention readout: softmax weights of one query row per sequence, summed per key segment ----
 * What output_attentions=True of a transformers decoder gives for the last prompt row, reduced to what a few-shot study reads:
 * how much of the row's attention falls on each piece of the prompt.  V is never read.
 *   Q      bf16, already rotated (and normalised, for a QK-norm decoder); head h of sequence b at column h * head_dim of row
 *          q_rows[b] (q_rows NULL: row b).  ldq % 8 == 0, ldq >= n_heads * head_dim.
 *   Kc     the bf16 K cache of the decode kernels, [n_seqs][n_kv_heads][max_len][head_dim]; query head h reads K/V head
 *          h / (n_heads / n_kv_heads); n_kv_heads 0 = n_heads.  Rows at or past lens[b] (>= 1) are never read.
 *   seg    seg[b * ld_seg + j] = the segment of key j; an id >= n_seg counts nowhere; entries at or past lens[b] are never read.
 *   s_j = scale * sum_d q_d k_jd (f32),  p_j = exp(s_j - max s) / sum_i exp(s_i - max s),
 *   mass[b][h][g] = sum_{j < lens[b], seg_j = g} p_j  (f32 [n_seqs][n_heads][n_seg]; a segment without a key is exactly 0.0f),
 *   probs[b][h][j] = p_j for j < lens[b] (f32 [n_seqs][n_heads][ld_probs], the rest untouched), or NULL.
 * head_dim 64 or 128 multi-head; grouped (2 <= G <= 8 query heads per K/V head) at head_dim 128, one workgroup per (sequence,
 * K/V head) loading a key row once for its G heads.  Two passes over K: the bytes of one icl_attn_decode_bf16 launch.
 * No atomics, every sum in a fixed order that depends on the sequence's own length only: a row's mass and probs are
 * bit-identical alone and in any batch.
 * ICL_EINVAL (before any launch): a NULL Q / Kc / lens / seg / mass, n_seg outside 1..32, head_dim not 64 / 128, n_kv_heads not
 * dividing n_heads, G > 8, G > 1 at head_dim 64, ld_seg < max_len, probs with ld_probs < max_len, a scale that is not finite.
 */
int icl_attn_segmass_bf16(const void* Q, int64_t ldq, const int32_t* q_rows, const void* Kc, const int32_t* lens,
                          const uint8_t* seg, int64_t ld_seg, int32_t n_seg, float* mass, float* probs, int64_t ld_probs,
                          int32_t n_seqs, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, int32_t max_len, float scale,
                          void* stream);

/* ---- segment-to-segment attention flow: the causal softmax weights of EVERY prompt row, summed by (query segment, key segment) ----
 * The descriptive side of the cuts below, and the readout above for all rows at once: what output_attentions=True of a transformers
 * decoder (eager attention) gives as an S x S matrix per layer and head, summed by (seg[i], seg[j]).  Replaces that matrix and the
 * loop of one-row icl_attn_segmass_bf16 launches it would otherwise take.  V is never read.
 *   Q      bf16, packed rotated query rows (normalised, for a QK-norm decoder): row cu[b] + i is position i of sequence b, head h at
 *          column h * head_dim.  ldq % 8 == 0, ldq >= n_heads * head_dim.
 *   cu     int32 [n_seqs + 1], ascending: sequence b has len = cu[b + 1] - cu[b] positions, 1 <= len <= max_seqlen <= max_len.
 *   Kc     the bf16 K cache of the decode kernels, [n_seqs][n_kv_heads][max_len][head_dim], holding positions 0 .. len - 1; query
 *          head h reads K head h / (n_heads / n_kv_heads); n_kv_heads 0 = n_heads.  Rows at or past len are never read.
 *   seg    seg[b * ld_seg + i] = the segment of position i, as a query row and as a key; entries at or past len are never read.
 *   p(i, j) = softmax over j <= i of scale * sum_d q_id k_jd,
 *   flow[b][h][a][c] = sum_{i < len, seg_i = a} sum_{j <= i, seg_j = c} p(i, j)    (f32 [n_seqs][n_heads][n_seg][n_seg], compact).
 * An id >= n_seg on a query row: the row is summed nowhere; on a key: it counts in no segment but stays in the row's softmax.
 * Every element of flow is written (no zero-fill contract); a pair (a, c) with no (i, j) to count is exactly 0.0f.
 * Flash-shaped: S^T = K Q^T on MFMA with the query on the lane, keys in tiles of 64 through LDS, an online (m, l) per lane; the
 * P V product is P E with E the one-hot [key][segment] matrix built in registers, P as a two-term bf16 split (hi + lo).  One
 * workgroup per (sequence, query head) walks the 128-query blocks in order.  No atomics, every sum in a fixed order that depends on
 * the sequence's own length and ids only: a sequence's flow is bit-identical alone and in any batch.
 * head_dim 64 or 128 multi-head; grouped (2 <= G <= 8 query heads per K/V head) at head_dim 128.
 * ICL_EINVAL (before any launch, naming the argument): a NULL Q / cu / Kc / seg / flow, n_seg outside 1..32, head_dim not 64 / 128,
 * n_kv_heads not dividing n_heads, G > 8, G > 1 at head_dim 64, n_seqs outside 1..65535, max_seqlen outside 1..max_len,
 * ld_seg < max_len, ldq % 8 or ldq < n_heads * head_dim, misaligned Q / Kc (16 B) or flow (4 B), a scale that is not finite.
 */
int icl_attn_segflow_bf16(const void* Q, int64_t ldq, const int32_t* cu, const void* Kc, const uint8_t* seg, int64_t ld_seg,
                          int32_t n_seg, float* flow, int32_t n_seqs, int32_t n_heads, int32_t n_kv_heads /* 0 = n_heads */,
                          int32_t head_dim, int32_t max_len, int32_t max_seqlen, float scale, void* stream);

/* ---- attention knockout: icl_attn_decode_bf16 / icl_attn_decode_gqa_bf16 over a row LIST, under a per-key segment mask ----
 * The causal companion of the readout above: the deciding query attends as if chosen pieces of the prompt were not there.
 * List entry r (0 <= r < n_rows) works on cache sequence row_seq[r]: it reads the query (bf16, already rotated) at row row_q[r]
 * of Q and writes row row_q[r] of O; rows of O that no entry lists are not written.  row_seq values must be sequences of the
 * cache and of lens / seg, row_q values rows of Q / O (the caller's duty: the call cannot see those extents).
 *   Kc/Vc  the bf16 cache of the decode kernels, [n_seqs][n_kv_heads][max_len][head_dim]; n_kv_heads 0 = n_heads.
 *   seg    seg[row_seq[r] * ld_seg + j] = the segment of key j (u8); entries at or past lens[row_seq[r]] are never read.
 *   blocked  u32 [n_rows][n_heads]: bit g of blocked[r * n_heads + h] = query head h of entry r does not read segment g.
 *   Key j counts for head h iff j < lens[row_seq[r]] and not (seg_j < 32 and bit seg_j of the mask): ids >= 32 are never blocked.
 * The softmax runs over the keys that count, in the stream order of the unmasked kernel (a key that does not count is a key past
 * the end): a mask of 0 gives icl_attn_decode_bf16's sums in its stream order (within rounding of that call, not bit-equal to it
 * by contract), a (row, head) without a key that counts writes zeros (the L > 0 rule).  One instantiation per (head_dim, G)
 * whatever n_rows is: a row's output is bit-identical alone and in any list.  One byte per key is read on top of a decode launch.
 * head_dim 64 or 128 multi-head; grouped (2 <= G <= 8) at head_dim 128, each head's own mask on the K / V chunk its group shares.
 * ICL_EINVAL (before any launch, naming the argument): a NULL pointer, n_rows <= 0 (or > 65535), head_dim not 64 / 128,
 * n_kv_heads not dividing n_heads, G > 8, G > 1 at head_dim 64, ld_seg < max_len, misaligned Q / Kc / Vc (16 B; ldq % 8),
 * ldq / ldo < n_heads * head_dim, a scale that is not finite.
 */
int icl_attn_decode_masked_bf16(const void* Q, int64_t ldq, const void* Kc, const void* Vc, void* O, int64_t ldo,
                                const int32_t* lens, const uint8_t* seg, int64_t ld_seg, const uint32_t* blocked,
                                const int32_t* row_seq, const int32_t* row_q, int32_t n_rows, int32_t n_heads, int32_t n_kv_heads,
                                int32_t head_dim, int32_t max_len, float scale, void* stream);

/* ---- attention cuts between prompt segments: the masked kernel over TILES of listed rows of one cache sequence ----
 * The knockout above rewrites one row per sequence; an edge whose QUERY is an interior prompt row ("the label positions may not
 * read their demonstration's text") lists hundreds.  A tile t (0 <= t < n_tiles) holds tile_rows = R slots, all of cache
 * sequence tile_seq[t]; slot e = t * R + r reads the query (bf16, already rotated) at row row_q[e] of Q and writes row row_q[e] of
 * O (row_q[e] < 0: an empty slot, nothing read or written).  One workgroup per (K/V head, tile) walks keys 0 .. max row_len of its
 * live slots - 1 ONCE for its R slots (and the G query heads of the group):
 *   key j counts for slot e iff j < row_len[e] (its query's position + 1: the causal bound) and not (seg_j < 32 and bit seg_j of
 *   blocked[e]); seg[tile_seq[t] * ld_seg + j] is the segment of key j, ids >= 32 are never blocked.
 *   head_on  u8 [n_heads] or NULL (all): a query head that is off is NOT written; a K/V group whose heads are all off does nothing.
 * The softmax runs over the keys that count, in the stream order of the decode kernels; a live slot without a key that counts
 * writes zeros.  R is a property of the form — icl_attn_cut_tile_rows: 4 for multi-head (head_dim 64 / 128), 2 for G = 2, 1 for
 * G = 3 .. 8 (head_dim 128), -1 for a form the kernel does not have — and one instantiation serves a form whatever n_tiles is: a
 * slot's output bits do not depend on its slot, its companions or the grid.  Rows of one tile should be close in row_len (the
 * tile streams up to its longest); row_q / tile_seq values must be rows of Q / O and sequences of the cache (the caller's duty).
 * ICL_EINVAL (before any launch, naming the argument): a NULL pointer but head_on, n_tiles outside 1..65535, tile_rows not the
 * form's R, head_dim not 64 / 128, n_kv_heads not dividing n_heads, G > 8, G > 1 at head_dim 64, ld_seg < max_len, ldq / ldo <
 * n_heads * head_dim, misaligned Q / Kc / Vc (16 B; ldq % 8) or blocked (4 B), a scale that is not finite.
 */
int icl_attn_cut_tile_rows(int32_t n_heads, int32_t n_kv_heads /* 0 = n_heads */, int32_t head_dim);
int icl_attn_cut_rows_bf16(const void* Q, int64_t ldq, const void* Kc, const void* Vc, void* O, int64_t ldo,
                           const uint8_t* seg, int64_t ld_seg, const int32_t* tile_seq, const int32_t* row_q,
                           const int32_t* row_len, const uint32_t* blocked, const uint8_t* head_on, int32_t n_tiles,
                           int32_t tile_rows, int32_t n_heads, int32_t n_kv_heads /* 0 = n_heads */, int32_t head_dim,
                           int32_t max_len, float scale, void* stream);

/* ---- K11: the decode step's RoPE + KV-cache append + attention as ONE launch --------------------
 * icl_rope_kv_bf16 (M = n_seqs rows, one new position each) followed by icl_attn_decode_bf16, fused: qkv bf16 [n_seqs][ld] holds
 * the QKV projection's raw q | k | v row of every sequence (column blocks at 0 | k_off | v_off, n_heads*head_dim wide);
 * for sequence b the kernel rotates q and k at position pos[b] (cos / sin f32 [max_pos][head_dim/2]), appends the rotated k
 * and v to cache row seq_ids[b] (NULL: b) at position pos[b], and attends over lens[b] = pos[b] + 1 keys — the appended
 * one taken from registers.  Same rounding points as the two calls (rope_rot8, bf16 q / k): bit-identical output and cache.
 * The qkv buffer is NOT modified (icl_rope_kv_bf16 rotates it in place; nothing reads it afterwards).
 * Replaces apply_rotary_pos_emb + DynamicCache.update + the attention of transformers' LlamaAttention in a decode step
 * (HF generate loop behind models/custom_salmon.py:704-720).
 */
int icl_attn_decode_rope_bf16(const void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const float* cos, const float* sin,
                              const int32_t* pos, const int32_t* seq_ids, void* kcache, void* vcache, void* O, int64_t ldo,
                              const int32_t* lens, int32_t n_seqs, int32_t n_heads, int32_t head_dim, int32_t max_len,
                              float scale, void* stream);

/* ---- K3/K5/K6/K7: LayerNorm;  K10/K14: RMSNorm -----------------------------------------
 * LayerNorm: v = x[m][:] + (res ? alpha * res[m][:] : 0);
 *            y[m][:] = (v - mean(v)) * rsqrt(var(v) + eps) * gamma + beta   (biased variance)
 *   The optional pre-add is BEATs' deep-norm post-LN, LN(x + alpha*residual) (K5); res has
 *   dtype in_dtype and leading dimension ldx.  y2 (optional, bf16, leading dimension ldy2)
 *   receives a second copy of y: post-LN blocks (BEATs, Q-Former) keep the f32 stream in y
 *   and feed the next GEMM from y2.
 * RMSNorm:   y[m][:] = x[m][:] * rsqrt(mean(x^2) + eps) * gamma
 * x is f32 or bf16 (in_dtype), y bf16 or f32 (out_dtype); gamma/beta f32; all math in f32;
 * N % 4 == 0 and N <= 8192.
 * Replaces nn.LayerNorm / LlamaRMSNorm in the HF / SALMONN modules (models/custom_salmon.py
 * :550-554, :630-636) incl. SALMONN's ln_speech / ln_audio (K6).
 */
int icl_layernorm(const void* x, int64_t ldx, const void* res, float alpha, const float* gamma,
                  const float* beta, void* y, int64_t ldy, void* y2, int64_t ldy2, int32_t M,
                  int32_t N, float eps, int32_t in_dtype, int32_t out_dtype, void* stream);
int icl_rmsnorm(const void* x, int64_t ldx, const float* gamma, void* y, int64_t ldy, int32_t M,
                int32_t N, float eps, int32_t in_dtype, int32_t out_dtype, void* stream);

/* ---- K10/K11/K14: rotary embedding + KV-cache append -------------------------------------
 * In place on the q and k column blocks of a fused bf16 QKV buffer [M][ld] (q at column 0,
 * k at column k_off, v at column v_off; n_heads x head_dim each; HF "rotate_half" pairing
 * (i, i+head_dim/2)); cos/sin f32 [max_pos][head_dim/2].  Row m belongs to sequence seq_ids[m]
 * at position pos[m].  If kcache != NULL the rotated k and the v row are also written to the
 * cache ([n_seqs][n_heads][max_len][head_dim]) at row pos[m] of sequence seq_ids[m].
 * Replaces LlamaRotaryEmbedding/apply_rotary_pos_emb + DynamicCache.update of transformers,
 * reached from models/custom_salmon.py:630-636 / :704-720.
 */
int icl_rope_kv_bf16(void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const float* cos,
                     const float* sin, const int32_t* pos, const int32_t* seq_ids, void* kcache,
                     void* vcache, int32_t M, int32_t n_heads, int32_t head_dim, int32_t max_len,
                     void* stream);

/* icl_rope_kv_bf16 for grouped-query attention: the q block has n_heads heads, the k / v blocks (at k_off / v_off) and the
 * cache ([n_seqs][n_kv_heads][max_len][head_dim]) n_kv_heads.  The same kernel, rotation and rounding points; with
 * n_kv_heads == n_heads it is icl_rope_kv_bf16.  The column blocks must be disjoint inside a row. */
int icl_rope_kv_gqa_bf16(void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const float* cos,
                         const float* sin, const int32_t* pos, const int32_t* seq_ids, void* kcache,
                         void* vcache, int32_t M, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim,
                         int32_t max_len, void* stream);

/* ---- K10/K11/K14: per-head q / k RMSNorm + rotary embedding + KV-cache append (QK-norm decoders: Qwen3) ----------
 * icl_rope_kv_gqa_bf16 with an RMSNorm over head_dim on every q head row and every k head row in front of the rotation; the
 * contract is that call's in everything the two share (in-place q / k, the append of k and v to
 * [n_seqs][n_kv_heads][max_len][head_dim], caches NULL together, disjoint column blocks).  head_dim 64 or 128;
 * q_gamma / k_gamma f32 [head_dim], shared by all heads; eps > 0.  For a head row x (bf16) of q or k:
 *     ss   = sum_i x[i]^2 in f32: each of the head_dim / 8 lanes of the row adds its eight squares in element order, the
 *            partial sums are folded by an xor butterfly over lane distances 1, 2, .. head_dim / 16
 *     r    = rsqrtf(ss * (1 / head_dim) + eps)
 *     n[i] = bf16_rne((x[i] * r) * gamma[i])            gamma = q_gamma for q rows, k_gamma for k rows
 * and n goes through rope_rot8 exactly as icl_rope_kv_gqa_bf16 rotates a buffer holding n (non-contracted IEEE arithmetic:
 * that stage is bit-defined).  One bf16 rounding point sits between the norm and the rotation, where a bf16 execution of the
 * HF module rounds too.  An all-zero row gives zeros; the domain is |x| <= 2^60.  v is copied to the cache untouched.
 * Replaces Qwen3Attention's q_norm / k_norm (Qwen3RMSNorm over head_dim) + apply_rotary_pos_emb + DynamicCache.update of
 * transformers, reached from models/custom_salmon.py:630-636 / :704-720.
 */
int icl_qknorm_rope_kv_bf16(void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const float* q_gamma,
                            const float* k_gamma, float eps, const float* cos, const float* sin, const int32_t* pos,
                            const int32_t* seq_ids, void* kcache, void* vcache, int32_t M, int32_t n_heads,
                            int32_t n_kv_heads, int32_t head_dim, int32_t max_len, void* stream);

/* ---- K10/K11: QKV projection with RoPE + KV-cache append fused into its epilogue -----------
 * icl_gemm_bf16(args) followed by icl_rope_kv_bf16 on its output, as ONE kernel: the 256x256 tile
 * stages its bf16 C tile through LDS, and with head_dim = 128 a tile is two whole heads of q, k or
 * v, so the row phase rotates (q, k), stores the rows and appends k/v to the cache — the QKV rows
 * are not read back from HBM.  Bit-identical to the two-call sequence (same rounding points).
 * args: batch 1, bf16 output, epilogue 0 or ICL_EPI_BIAS, N = 3*n_heads*128 with q|k|v column
 * blocks at 0 | k_off | v_off, n_heads*128 a multiple of 256; the problem must resolve to the
 * 256x256 tile (icl_gemm_select_tile(...) == 3 and K >= 128, or args->tile = 3) — otherwise ICL_EINVAL, and the
 * caller issues the two calls.  A section may be EMPTY: a launch over the k | v rows of the weight alone has k_off = 0,
 * v_off = n_heads*128, N = 2*n_heads*128; one over its q rows alone has k_off = v_off = N = n_heads*128 (the last decoder
 * layer of a prefill projects k / v for every row and q for the last row of each sequence only).  Remaining arguments as icl_rope_kv_bf16.  kv_rows_to_c = 0 (needs a cache): the k / v
 * column blocks of C are NOT written — they exist only in the cache, where icl_attn_fwd_bf16 can read them
 * (kv_seq_stride / kv_head_stride); q is always written.
 * Replaces q_proj/k_proj/v_proj + apply_rotary_pos_emb + DynamicCache.update of transformers'
 * LlamaAttention, reached from models/custom_salmon.py:630-636 (prefill).
 */
int icl_gemm_rope_kv_bf16(const icl_gemm_args* args, int64_t k_off, int64_t v_off, const float* cos,
                          const float* sin, const int32_t* pos, const int32_t* seq_ids, void* kcache,
                          void* vcache, int32_t n_heads, int32_t head_dim, int32_t max_len, int32_t kv_rows_to_c,
                          void* stream);

/* ---- K9: token-embedding gather + speech interleave --------------------------------------
 * out[r][:] = src_idx[r] >= 0 ? table[src_idx[r]][:] : speech[-src_idx[r]-1][:]
 * table bf16 [vocab][H]; speech f32 [n_speech_rows][H]; out f32 [rows][H].
 * Replaces embed_tokens + torch.cat interleave of models/custom_salmon.py:189-194, :243-283.
 */
int icl_embed_gather_interleave(const int32_t* src_idx, const void* table, const float* speech,
                                float* out, int32_t rows, int32_t H, int32_t vocab,
                                int32_t n_speech_rows, void* stream);

/* ---- K11: greedy argmax + EOS/pad bookkeeping --------------------------------------------
 * tok = finished[b] ? pad_id : argmax_v logits[b][v] (lowest index on ties);
 * finished[b] |= (tok == eos_id || tok == eos_id2); out_tokens[b*out_stride + step] = tok; next_ids[b] = tok.
 * eos_id2 = -1 when the generation config names one EOS id (HF accepts a list: Qwen2-Audio's is [151643, 151645]).
 * Replaces HF GenerationMixin._sample greedy branch (models/custom_salmon.py:704-720).
 */
int icl_argmax_eos(const float* logits, int64_t ldl, int32_t B, int32_t V, int32_t eos_id, int32_t eos_id2,
                   int32_t pad_id, int32_t* finished, int32_t* out_tokens, int32_t out_stride,
                   int32_t step, int32_t* next_ids, void* stream);

/* ---- K11 (constrained): greedy argmax along a token automaton + EOS/pad bookkeeping + log-probability ----
 * The automaton is CSR: the edges of state s are state_off[s] .. state_off[s+1] - 1, sorted by edge_tok and unique, edge e
 * leads to edge_next[e]; state_dist[s] = the fewest tokens from s to an accepting state (one with an edge on the EOS id).
 * The tables are trusted: the caller validates them before the upload (offsets monotone, tokens in [0,V), next states in
 * [0,n_states)).  Per row b (state[b] is read and written; steps_left = the tokens the row may still emit, this one included):
 *   finished[b]                     tok = pad_id, out_logprob = 0, state[b] untouched;
 *   state[b] == -1 (a free row; any id outside [0,n_states) is treated the same and is never used as an index):
 *                                   tok = icl_argmax_eos's (lowest index on ties, a NaN logit cannot be chosen and carries no
 *                                   mass); out_logprob = logits[b][tok] - log-sum-exp over the whole row;
 *   otherwise                       candidates = the edges e of state[b] with state_dist[edge_next[e]] <= steps_left - 1; tok =
 *                                   the edge_tok of the candidate with the largest logit (NaN counts as -inf; the lowest token
 *                                   id on ties, hence the first candidate when all are -inf); state[b] = its edge_next;
 *                                   out_logprob = its logit - log-sum-exp over the candidates.
 * Log-sum-exp is f32 with the maximum subtracted first; out_logprob is NaN where that is undefined (no finite candidate, or a
 * +inf one).  A constrained row without any candidate (the caller broke steps_left >= state_dist[state[b]]) ends: tok = pad_id,
 * finished[b] = 1, out_logprob = NaN.  Then icl_argmax_eos's bookkeeping word for word: finished[b] |= tok is an EOS id;
 * out_tokens[b*out_stride + step] = next_ids[b] = tok.  out_logprob is NULL or f32 [B][out_stride], written at the same index.
 * One workgroup per row, one pass over the row (free) or over one state's edges (constrained); nothing allocates or
 * synchronises, so the launch can be captured in a graph.  No counterpart in the reference, which repairs free-running
 * output on the host afterwards (utils/evaluation_utils.py clean_prediction).
 */
int icl_argmax_fsm(const float* logits, int64_t ldl, int32_t B, int32_t V, const int32_t* state_off, const int32_t* edge_tok,
                   const int32_t* edge_next, const int32_t* state_dist, int32_t n_states, int32_t n_edges, int32_t* state,
                   int32_t steps_left, int32_t eos_id, int32_t eos_id2, int32_t pad_id, int32_t* finished,
                   int32_t* out_tokens, int32_t out_stride, int32_t step, int32_t* next_ids, float* out_logprob,
                   void* stream);

/* ---- K11 (sampled): repetition penalty -> temperature -> top-k -> top-p -> inverse-CDF draw + EOS/pad bookkeeping ----
 * Per sequence b: scores = logits[b] with every token in prev_tokens[b][0..n_prev) rescaled (x<0 ? x*penalty : x/penalty),
 * all divided by temperature; candidates = scores >= the top_k-th largest score (ties kept); probabilities = softmax over
 * the candidates sorted by (score desc, token asc); candidate j is dropped when the mass of candidates j.. is <= 1-top_p
 * (the largest always stays); the token is the first kept candidate whose running mass exceeds uniforms[b] * kept mass.
 * Then exactly icl_argmax_eos's bookkeeping.  work f32 [B][ldw>=V] is scratch; top_k in [1,1024], or top_k == V = "top-k
 * off" (HF: top_k 0 / None): probabilities are then normalised over the whole row, candidates are the 1024 most likely
 * tokens and a nucleus wider than that is truncated to them; any other top_k is ICL_EINVAL.  Greedy search with a
 * repetition penalty is top_k = 1.  Optional debug outputs (NULL to skip): the kept tokens, their renormalised
 * probabilities and their count, dbg_cap entries per sequence.
 * Overflow rule: the candidate list has 1024 slots.  When more than 1024 tokens are at or above the cut (ties at the cut: a
 * flat row, a row masked with -inf that leaves fewer finite scores than top_k, top-k off with ties at the 1024th value),
 * the list holds EVERY token strictly above the cut, then the tied tokens by ascending token id until it is full — the
 * first 1024 tokens in (score desc, token asc) order, the same on every launch.  Probabilities are finite whenever the row
 * has a finite score: a -inf score has probability 0 and is never drawn, and neither is a NaN score (NaN sorts below -inf;
 * one that reaches the list — fewer comparable scores than top_k, or top-k off — carries no mass).
 * Replaces HF generate(do_sample=True, temperature, top_p, repetition_penalty) as called at models/custom_salmon.py:705-721
 * (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper [generation-config default 50],
 * TopPLogitsWarper, softmax, multinomial).
 */
int icl_sample_eos(const float* logits, int64_t ldl, int32_t B, int32_t V, float* work, int64_t ldw,
                   const int32_t* prev_tokens, int32_t prev_stride, int32_t n_prev, float repetition_penalty,
                   float temperature, int32_t top_k, float top_p, const float* uniforms, int32_t eos_id, int32_t eos_id2,
                   int32_t pad_id, int32_t* finished, int32_t* out_tokens, int32_t out_stride, int32_t step,
                   int32_t* next_ids, int32_t* dbg_ids, float* dbg_probs, int32_t* dbg_count, int32_t dbg_cap,
                   void* stream);

/* ---- K1: Whisper log-mel (f64 STFT, f32 out) ---------------------------------------------
 * wav f32 [n_audio][wav_ld] with valid lengths wav_lens (device int32; samples past the length
 * or past 480000 are treated as zero), -> spec f32 [n_audio][80][3000] (n_mel x 3000) and,
 * if xt != NULL, the conv-stem operand bf16 [n_audio][3002][xt_ld] (time-major, rows 0 and
 * 3001 zero, columns >= n_mel zero).  n_fft=400, hop=160, periodic Hann, reflect-padded
 * centre frames, Slaney mel filters `mel_filters` f64 [n_mel][201], log10, max-8 clamp,
 * (x+4)/4 — WhisperFeatureExtractor semantics (data/model_processors.py:641-645, :659-663).
 * workspace: f32 [n_audio][n_mel][3000] + int32 [n_audio] (raw log10 values + per-audio max).
 */
int icl_logmel_whisper(const float* wav, int64_t wav_ld, const int32_t* wav_lens,
                       const double* mel_filters, int32_t n_mel, int32_t n_audio, float* spec,
                       void* xt, int64_t xt_ld, void* workspace, void* stream);
/* spec f32 [n_audio][n_mel][3000] -> conv-stem operand xt (same layout as above). */
int icl_spec_to_xt(const float* spec, int32_t n_mel, int32_t n_audio, void* xt, int64_t xt_ld,
                   void* stream);

/* ---- K4: BEATs front-end: Kaldi fbank (f64 math, f32 out) ---------------------------------
 * wav (f32, scaled by 2^15 inside) -> fbank f32 [n_audio][max_frames][128]:
 * 25 ms / 10 ms frames (snip_edges), DC removal, pre-emphasis 0.97, povey window, 512-pt
 * power spectrum, 128 Kaldi mel bins (`mel_banks` f64 [128][257]), log(max(x, FLT_EPSILON)),
 * then (x - mean) / (2*std).  Frames >= n_frames(len) are written as the value the reference
 * produces for zero-padded audio only when `wav` itself holds those zeros; rows past
 * max_frames are not touched.  torchaudio.compliance.kaldi.fbank semantics as used by
 * BEATs.preprocess (external SALMONN package; call site models/custom_salmon.py:412-416).
 */
int icl_fbank_kaldi(const float* wav, int64_t wav_ld, const int32_t* wav_lens,
                    const double* mel_banks, int32_t n_audio, int32_t max_frames, float mean,
                    float std, float* fbank, void* stream);

/* ---- K7: window-level Q-Former cross attention (1 query x win keys) ------------------------
 * q bf16 [n_win][ldq] (n_heads x 64), kv bf16 [n_audio*rows_per_audio][ldkv] with K at
 * column 0 and V at column v_off; window w of audio a covers rows a*rows_per_audio + w*win
 * .. +win-1 (SALMONN's F.unfold with kernel == stride is a free view).
 * out bf16 [n_win][ldo].  Replaces BertSelfAttention(cross) of SALMONN's speech_Qformer
 * (call site models/custom_salmon.py:550-554).
 */
int icl_qformer_window_xattn(const void* q, int64_t ldq, const void* kv, int64_t ldkv,
                             int64_t v_off, void* out, int64_t ldo, int32_t n_audio,
                             int32_t win_per_audio, int32_t win, int32_t rows_per_audio,
                             int32_t n_heads, float scale, void* stream);

/* ---- small fused element-wise helpers ----------------------------------------------------- */
/* BEATs gate (K5): from the fused bf16 QKV rows (q block = first n_heads*64 columns, WITH
 * bias, unscaled), gate[m][h] = ga*(gb*grep_a[h]-1)+2 where (ga,gb) =
 * sigmoid(sum4(grep_w[8][64]·q_h + grep_b[8])).  Output f32 [M][n_heads]. */
int icl_beats_gate(const void* qkv, int64_t ld, const float* grep_w, const float* grep_b,
                   const float* grep_a, float* gate, int32_t M, int32_t n_heads, void* stream);
/* y = x (+ y_in) with dtype conversion: out[m][n] = (float)in[m][n] * alpha (+ add[m][n]) */
int icl_axpby_cast(const void* in, int64_t ldi, int32_t in_dtype, const void* add, int64_t lda_,
                   int32_t add_dtype, float alpha, void* out, int64_t ldo, int32_t out_dtype,
                   int32_t M, int32_t N, void* stream);
/* LoRA down-projection written into the K-augmentation columns of the GEMM operand:
 * X[m][K0 + j] = bf16( scale * sum_k X[m][k] * A[j][k] ), j < r_total; A bf16 [r_total][lda_].
 * (peft LoRA restated: W x + (alpha/r) B (A x); models/custom_salmon.py:78-81 config.) */
int icl_lora_down_bf16(void* X, int64_t ldx, int32_t K0, const void* A, int64_t lda_,
                       int32_t r_total, float scale, int32_t M, void* stream);

/* ---- K4/K5: BEATs data movers (so both BEATs convolutions run on icl_gemm_bf16) ----------------
 * icl_beats_patchify: fbank f32 [n_audio][max_frames][128] -> im2col of Conv2d(1->512, k=16, s=16):
 *   out bf16 [total_rows][256], packed row cu_rows[a] + t'*8 + f', column i*16 + j =
 *   fbank[a][16t'+i][16f'+j]  (BEATs.patch_embedding; external SALMONN package, call site
 *   models/custom_salmon.py:412-416).
 * icl_beats_posconv_pack: x f32 [total_rows][channels] (packed by cu_rows; BEATs: 768 channels, 16 groups).  Rows >= valid_rows[a] of
 *   audio a are zeroed in place (backbone `x[padding_mask] = 0`), and xg (bf16) receives per audio
 *   the image [groups][T_a + 128][channels/groups] with 64 zero rows in front / 64 behind, located at
 *   element offset (cu_rows[a] + 128*a)*channels: row t of group g then sees the 128x48 taps of
 *   Conv1d(768,768,k=128,pad=64,groups=16) as ONE contiguous K = 6144 run (lda = 48).
 * icl_gather_rows_f32 / icl_gather_rows_bf16: out[r][:] = src[idx[r]][:]  (last-token rows for the LM head; the rows the last
 *   decoder layer of a prefill keeps).  16-byte moves: N and the leading dimensions are multiples of 4 (f32) / 8 (bf16).
 */
int icl_beats_patchify(const float* fbank, int32_t max_frames, const int32_t* cu_rows, int32_t n_audio,
                       int32_t total_rows, void* out, void* stream);
int icl_beats_posconv_pack(float* x, const int32_t* cu_rows, const int32_t* valid_rows, int32_t n_audio,
                           int32_t total_rows, int32_t channels, int32_t groups, void* xg, void* stream);
int icl_gather_rows_f32(const float* src, int64_t ld_src, const int32_t* idx, float* out, int64_t ld_out,
                        int32_t rows, int32_t N, void* stream);
int icl_gather_rows_bf16(const void* src, int64_t ld_src, const int32_t* idx, void* out, int64_t ld_out,
                         int32_t rows, int32_t N, void* stream);

/* ---- residual-stream capture and patching at listed rows ------------------------------------------------------------
 * The read and the write of an in-context-learning study on the f32 residual stream h [.][ldh] (transformers:
 * output_hidden_states=True plus a forward pre-hook on a decoder layer).  List entry r (0 <= r < n_rows) works on row
 * row = rows[r] of h, for 0 <= i < hidden, in this order:
 *   capture (unless NULL):  capture[r*ld_cap + i] = h[row*ldh + i], copied as bits: always the value BEFORE the patch;
 *   vec (unless NULL), entry r's vector at vec + r*ld_vec (ld_vec == 0: one vector for all entries):
 *     mode 0, replace:  h[row*ldh + i] = vec[r*ld_vec + i], copied as bits (NaN payloads, -0.0 and subnormals survive);
 *     mode 1, add:      h[row*ldh + i] = __fmaf_rn(alpha, vec[r*ld_vec + i], h[row*ldh + i]): ONE rounding, of the exact
 *                       alpha*v + h (not a rounded product and a rounded sum).  Mode 0 does not use alpha (still checked).
 * Rows that no entry lists, and the columns of a listed row at or beyond hidden, are not written.  rows values must be rows of
 * h (the caller's duty: the call cannot see that extent); a row listed TWICE is the caller's error — two blocks would race on
 * it — and the host layers above refuse such lists.  capture and vec must not overlap h.  One block per entry, 16-byte moves,
 * all address arithmetic in int64_t (ldh may exceed 2^32).
 * ICL_EINVAL (before any launch, naming the argument): h or rows NULL; capture and vec both NULL; n_rows outside 1..65535;
 * hidden <= 0 or not a multiple of 4; ldh, ld_cap (with capture) or a non-zero ld_vec (with vec) below hidden or not a multiple
 * of 4; h, capture or vec not 16-byte aligned; mode outside {0, 1}; alpha not finite.
 */
int icl_resid_rows_f32(float* h, int64_t ldh, const int32_t* rows, int32_t n_rows, int32_t hidden, float* capture,
                       int64_t ld_cap, const float* vec, int64_t ld_vec, int32_t mode, float alpha, void* stream);

/* ---- attention-head output capture and patching at listed rows -------------------------------------------------------
 * The read and the write of single heads' outputs — the D-vector a head hands to o_proj — on the bf16 attention-output buffer
 * att [.][ld_att] (transformers: a forward pre-hook on self_attn.o_proj).  Head h of a row is columns h*D .. h*D + D - 1,
 * D = head_dim.  List entry r (0 <= r < n_rows) works on row = rows[r] of att, in this order:
 *   capture (unless NULL):  capture[r*ld_cap + c] = att[row*ld_att + c] for c < n_heads*D, copied as bits (NaN payloads, -0.0
 *                           and subnormals survive): always the value BEFORE the patch;
 *   vec (unless NULL), for s < n_sel, h = heads[s], i < D, v = vec[r*ld_vec + s*D + i] (ld_vec == 0: one block of n_sel vectors
 *   for all entries), a = att[row*ld_att + h*D + i]:
 *     mode 0, replace:  a = bf16(v): f32_to_bf16_bits, round to nearest even, NaN stays NaN; a v that is a bf16 value comes back
 *                       as its bits;
 *     mode 1, add:      a = bf16(__fmaf_rn(alpha, v, (float)a)): ONE f32 rounding of the exact alpha*v + a, then the bf16 rounding.
 *                       Mode 0 does not use alpha (still checked).
 * Rows that no entry lists, heads that heads[] does not hold, and the columns at or beyond n_heads*D are not written.  rows values
 * must be rows of att (the caller's duty: the call cannot see that extent); heads values must be distinct and inside
 * 0..n_heads-1, and no row may be listed twice (two threads would race on it) — the host layers above refuse such lists.
 * capture and vec must not overlap att.  16-byte moves, one per thread; all address arithmetic in int64_t (ld_att may exceed 2^32).
 * ICL_EINVAL (before any launch, naming the argument): att or rows NULL; capture and vec both NULL; vec without heads; n_rows
 * outside 1..65535; head_dim not 64 or 128; n_heads outside 1..65535; with vec, n_sel outside 1..n_heads; ld_att or ld_cap (with
 * capture) below n_heads*D or not a multiple of 8; a non-zero ld_vec (with vec) below n_sel*D or not a multiple of 4; att,
 * capture or vec not 16-byte aligned; mode outside {0, 1}; alpha not finite.
 */
int icl_head_rows_bf16(void* att, int64_t ld_att, const int32_t* rows, int32_t n_rows, int32_t n_heads, int32_t head_dim,
                       void* capture, int64_t ld_cap, const int32_t* heads, int32_t n_sel, const float* vec, int64_t ld_vec,
                       int32_t mode, float alpha, void* stream);

/* ---- K11 (beam search): one step of HF's static-shaped beam search + the cache reorder ------------------------------
 * icl_beam_step, per batch row b (num_beams K <= 8, max_new_tokens T <= 64, V >= 2K): log-softmax of the K beams' logits
 *   (row b*rows_per_batch + k; rows_per_batch == 1 at step 0, where the K beams still share the prompt's one distribution) plus
 *   run_score[b][k]; the 2K best continuations (3K when eos_id2 >= 0: HF keeps (1 + number of EOS ids) * K; ties: lower
 *   beam*V + token); a continuation stops when its token is eos_id / eos_id2 or step + 1 == T.  run_* <- the K best that do not stop (score - 1e9 if only stopping ones are left); fin_* <- the K best of
 *   {old finished slots, first-K continuations that stop, scored sum / (step+1)**length_penalty}, taken only while unsat[b];
 *   unsat[b] &= (run_score[b][0] / (step+1)**length_penalty beats the worst finished slot, or a slot is still empty).
 *   next_ids[b*K+i] / parent[b*K+i] = token and absolute source row (b*K + parent beam) of running beam i.
 *   repetition_penalty != 1: the log-probability x of every token already in running beam k's sequence becomes x < 0 ? x * p : x / p
 *   before run_score is added (HF applies RepetitionPenaltyLogitsProcessor after log_softmax in beam search).
 *   Initial state: run_score = {0, -1e9, ...}, fin_score = -1e9, fin_flag = fin_len = 0, unsat = 1, sequences = pad.
 *   The answer after T steps is fin_seq[b][0][0 .. fin_len[b][0]).
 *   Replaces HF GenerationMixin._beam_search (early_stopping=False, do_sample=False) behind generate(inputs_embeds=...,
 *   num_beams, length_penalty) at models/custom_salmon.py:704-715 (per-task values: models/multi_task_model.py:142).
 * icl_kv_copy_spans_bf16: for every layer l < n_layers, head h < n_heads and row r < n_rows, copy n (= n_t[r], or n_fixed when
 *   n_t is NULL) positions of head_dim bf16 from src[l][src_seq[r]][h][src_t0[r] ..] to dst[l][dst_seq[r]][h][dst_t0[r] ..]
 *   (NULL seq array = r, NULL t0 array = 0; strides in elements).  src and dst spans must not overlap.  src / dst hold
 *   src_n_seqs / dst_n_seqs sequences of src_len / dst_len positions: ids, starts and counts read from device memory are
 *   clamped to those extents (ABI 5), so a corrupted parent id copies a wrong span, never out of bounds.  Stands in for HF's
 *   cache.reorder_cache(beam_idx): only the positions after the prompt differ between the beams of a row.
 *   icl_beam_step treats a NaN logit as -inf (a token that cannot be chosen; icl_argmax_eos does the same), so parent[]
 *   always names a beam of its own row.
 */
int icl_beam_step(const float* logits, int64_t ldl, int32_t rows_per_batch, int32_t B, int32_t V, int32_t num_beams,
                  int32_t max_new_tokens, int32_t step, int32_t eos_id, int32_t eos_id2, float length_penalty,
                  float repetition_penalty, float* run_score,
                  int32_t* run_seq, float* fin_score, int32_t* fin_seq, int32_t* fin_len, int32_t* fin_flag,
                  int32_t* unsat, int32_t* next_ids, int32_t* parent, void* stream);
int icl_kv_copy_spans_bf16(const void* src, void* dst, int64_t src_layer_stride, int64_t src_seq_stride,
                           int64_t src_head_stride, int64_t dst_layer_stride, int64_t dst_seq_stride,
                           int64_t dst_head_stride, const int32_t* src_seq, const int32_t* src_t0,
                           const int32_t* dst_seq, const int32_t* dst_t0, const int32_t* n_t, int32_t n_fixed,
                           int32_t n_rows, int32_t n_layers, int32_t n_heads, int32_t head_dim,
                           int32_t src_n_seqs, int32_t dst_n_seqs, int32_t src_len, int32_t dst_len, void* stream);

/* ---- K10/K11 (opt-in FP8 KV cache): fp8 append, decode attention and beam copy -------------------------------
 * Numeric contract.  A cache row x is one (layer, sequence, head, position) vector of head_dim elements: the post-RoPE key or the
 * value.  It is stored as head_dim OCP e4m3fn bytes q and one scale 2^e, where e is the smallest integer with
 * max_i |x[i]| <= 448 * 2^e (0 for an all-zero row) and q[i] = RNE_e4m3fn(x[i] / 2^e), never saturated: the bytes of
 * torch's (x.float() / 2**e).to(torch.float8_e4m3fn), the rule of icl_pack_fp8_weights per weight row.  x' = q * 2^e is exact in
 * bf16.  A row holding a non-finite element is stored as bytes 0x7f (NaN) with a NaN scale: all of it reads back as NaN.
 * Layout: bytes [n_seqs][n_heads][max_len][head_dim] (uint8) per layer, as the bf16 cache; scales f32 [n_seqs][n_heads][max_len]
 * (one f32 2^e per row, a plane of its own).  head_dim is 64 or 128.
 * The fp8-KV model is the bf16 model whose cache entries are replaced by x' when they are appended: prefill attends to its own
 * unrounded K/V (the caller runs the QKV GEMM with kv_rows_to_c and no bf16 append, then icl_kv_append_fp8), and every decode
 * step attends over x', the row appended in that step included.
 *
 * icl_kv_append_fp8: for every row m < M of qkv bf16 [M][ld] (k / v column blocks at k_off / v_off, already rotated), rounds
 *   the k and v of each head and stores them at (seq_ids[m], head, pos[m]).  A position outside [0, max_len) stores nothing.
 * icl_rope_kv_fp8: icl_rope_kv_bf16 with an fp8 cache: rotates q in place and k (rope_rot8, the same bf16 rounding points), and
 *   appends the rounded rotated k and v.  The k block of qkv is left unrotated (decode reads only q).
 * icl_attn_decode_fp8 / icl_attn_decode_rope_fp8: icl_attn_decode_bf16 / icl_attn_decode_rope_bf16 over an fp8 cache.  A
 *   lane reads 16 elements of a key row (one 16-byte load; head_dim / 16 lanes per row) and its scale, rebuilds x' exactly and
 *   runs the bf16 kernel's arithmetic (key groups, online softmax, merge) on it.  The output is bit-identical to
 *   icl_attn_decode_bf16_epl16 — the bf16 kernel instantiated with the same 16-element lane mapping, a reference entry point —
 *   on a bf16 cache holding x'; against icl_attn_decode_bf16 (8 elements per lane) only the order of each score's partial sums
 *   differs.  The fused form rounds the appended row in registers and attends over that rounded row.  A NaN row (see above) makes the output of its (sequence, head) NaN.
 * icl_kv_copy_spans_fp8: icl_kv_copy_spans_bf16 over both planes (byte strides for the row bytes, element strides for the
 *   scales); head_dim a multiple of 16.
 */
int icl_kv_append_fp8(const void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const int32_t* pos, const int32_t* seq_ids,
                      void* kq, void* vq, float* kscale, float* vscale, int32_t M, int32_t n_heads, int32_t head_dim,
                      int32_t max_len, void* stream);
int icl_rope_kv_fp8(void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const float* cos, const float* sin,
                    const int32_t* pos, const int32_t* seq_ids, void* kq, void* vq, float* kscale, float* vscale,
                    int32_t M, int32_t n_heads, int32_t head_dim, int32_t max_len, void* stream);
int icl_attn_decode_bf16_epl16(const void* Q, int64_t ldq, const void* Kc, const void* Vc, void* O, int64_t ldo,
                               const int32_t* lens, int32_t n_seqs, int32_t n_heads, int32_t head_dim, int32_t max_len,
                               float scale, void* stream);
int icl_attn_decode_fp8(const void* Q, int64_t ldq, const void* kq, const void* vq, const float* kscale, const float* vscale,
                        void* O, int64_t ldo, const int32_t* lens, int32_t n_seqs, int32_t n_heads, int32_t head_dim,
                        int32_t max_len, float scale, void* stream);
int icl_attn_decode_rope_fp8(const void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const float* cos, const float* sin,
                             const int32_t* pos, const int32_t* seq_ids, void* kq, void* vq, float* kscale, float* vscale,
                             void* O, int64_t ldo, const int32_t* lens, int32_t n_seqs, int32_t n_heads, int32_t head_dim,
                             int32_t max_len, float scale, void* stream);
int icl_kv_copy_spans_fp8(const void* src, const float* src_scale, void* dst, float* dst_scale, int64_t src_layer_stride,
                          int64_t src_seq_stride, int64_t src_head_stride, int64_t dst_layer_stride, int64_t dst_seq_stride,
                          int64_t dst_head_stride, int64_t src_scale_layer_stride, int64_t src_scale_seq_stride,
                          int64_t src_scale_head_stride, int64_t dst_scale_layer_stride, int64_t dst_scale_seq_stride,
                          int64_t dst_scale_head_stride, const int32_t* src_seq, const int32_t* src_t0, const int32_t* dst_seq,
                          const int32_t* dst_t0, const int32_t* n_t, int32_t n_fixed, int32_t n_rows, int32_t n_layers,
                          int32_t n_heads, int32_t head_dim, int32_t src_n_seqs, int32_t dst_n_seqs, int32_t src_len,
                          int32_t dst_len, void* stream);

/* ---- K12: causal-LM cross entropy (teacher-forced forward only) -------------------------------
 * row_loss[r] = logsumexp(logits[r][:]) - logits[r][labels[r]] for labels[r] in [0,V), else 0;
 * mean_loss[0] = mean of row_loss over the valid rows (NaN if none) — torch CrossEntropyLoss with
 * ignore_index=-100, reduction='mean'.  The caller passes row r = position t of a sequence together
 * with labels[r] = label of position t+1 (HF shift-by-one; models/custom_salmon.py:617-640).
 */
int icl_cross_entropy(const float* logits, int64_t ldl, const int32_t* labels, int32_t M, int32_t V,
                      float* row_loss, float* mean_loss, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICL_HIP_H */

// attn_segmass.hip — the prompt-attention readout: for ONE query row per sequence, the softmax weights over the K cache
// (optionally written out) and their sum over each segment of the keys.  V is never read.
// Cache layout and lane mapping are attn_decode.hip's: [n_seqs][n_kv_heads][max_len][D] bf16, D/8 lanes cover one key row with
// one 16-B load each straight to VGPRs, a wave-instruction fetches KPW = 64/(D/8) consecutive keys, and a workgroup of four waves
// per (sequence, K/V head) uses every key row it loads for all NG query heads of the group.
// Two passes over the keys (the bytes of one decode-attention launch, which reads K and V once each):
//   pass 1  every (wave, key slot) stream keeps an online (m, l) per head over its keys; the 4*KPW streams are merged once, in
//           stream order, into the row's maximum M and sum L;
//   pass 2  the scores are formed again by the same lanes with the same FMA chain (segmass_dot: explicit fmaf, nothing left to the
//           compiler's contraction, so a score has the bits pass 1 gave it), p_j = exp2(s_j - M) / L goes to `probs` and, a tile
//           of TK keys at a time, through LDS to the mass threads: thread (g, s) adds the tile's p_j of head g whose key lies in
//           segment s, in key order.
// Determinism: one instantiation per (D, NG) whatever the grid; which keys a stream folds, the merge order and the order of a
// segment's sum depend on the sequence's own length only — a row's mass and probs are the same bits alone and in any batch.
// No atomics.
#include "common.h"

namespace {

constexpr float SM_NEG_BIG = -1.0e30f;
constexpr float SM_LOG2E = 1.4426950408889634f;
constexpr int SM_MAX_SEG = 32;

// one lane's 8 elements of q . k, as a fixed chain of FMAs
__device__ __forceinline__ float segmass_dot(const float (&q)[8], u32x4 kw) {
  float d = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    d = fmaf(q[2 * t], __uint_as_float(kw[t] << 16), d);
    d = fmaf(q[2 * t + 1], __uint_as_float(kw[t] & 0xffff0000u), d);
  }
  return d;
}

// blockIdx.x = K/V head h (its query heads are h * NG + g), blockIdx.y = sequence b
template <int D, int NG>
__global__ __launch_bounds__(256) void attn_segmass_kernel(const unsigned short* Q, int64_t ldq, const int* q_rows,
                                                            const unsigned short* Kc, const int* lens, const unsigned char* seg,
                                                            int64_t ld_seg, int n_seg, float* mass, float* probs, int64_t ld_probs,
                                                            int n_kv_heads, int max_len, float scale_log2e) {
  constexpr int LPR = D / 8;          // lanes per key row
  constexpr int KPW = 64 / LPR;       // keys per wave-instruction
  constexpr int NSTREAM = 4 * KPW;    // (wave, key slot) streams of the block
  constexpr int U = 4;                // key rounds whose loads are issued together
  constexpr int TK = NSTREAM * U;     // keys per tile: 64 (D = 128) or 128 (D = 64)
  static_assert(NG >= 1 && NG <= 8 && NG * SM_MAX_SEG <= 256 && TK <= 256, "one mass thread per (head of the group, segment)");
  __shared__ float sm_m[NG][NSTREAM], sm_l[NG][NSTREAM], sm_ML[NG][2];
  __shared__ float pt[NG][TK];
  __shared__ int segt[TK];
  const int h = blockIdx.x, b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dc = lane % LPR, sub = lane / LPR;
  const int stream = wave * KPW + sub;
  const int len = min(lens[b], max_len);
  const int n_heads = n_kv_heads * NG;
  const int mg = threadIdx.x >> 5, ms = threadIdx.x & 31;     // the mass threads: head mg of the group, segment ms
  const bool mass_thread = mg < NG && ms < n_seg;
  float* mrow = mass + ((int64_t)b * n_heads + (int64_t)h * NG) * n_seg;
  if (len <= 0) {                                              // lens[b] >= 1 is the contract; nothing is read otherwise
    if (mass_thread) mrow[mg * n_seg + ms] = 0.f;
    return;
  }
  const unsigned short* kp = Kc + ((int64_t)b * n_kv_heads + h) * (int64_t)max_len * D + dc * 8;
  const unsigned short* qp = Q + (int64_t)(q_rows ? q_rows[b] : b) * ldq + (int64_t)h * NG * D + dc * 8;

  float q[NG][8];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const u32x4 w = *(const u32x4*)(qp + g * D);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      q[g][2 * t] = __uint_as_float(w[t] << 16) * scale_log2e;
      q[g][2 * t + 1] = __uint_as_float(w[t] & 0xffff0000u) * scale_log2e;
    }
  }

  // ---- pass 1: the row's maximum and sum
  float m[NG], l[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    m[g] = SM_NEG_BIG;
    l[g] = 0.f;
  }
  for (int j0 = 0; j0 < len; j0 += TK) {
    u32x4 kr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) kr[u] = *(const u32x4*)(kp + (int64_t)min(j0 + u * NSTREAM + stream, len - 1) * D);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      float s[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float d = segmass_dot(q[g], kr[u]);
#pragma unroll
        for (int x = 1; x < LPR; x <<= 1) d += __shfl_xor(d, x, 64);
        s[u] = j0 + u * NSTREAM + stream < len ? d : SM_NEG_BIG;
      }
      const float m_new = fmaxf(fmaxf(m[g], fmaxf(s[0], s[1])), fmaxf(s[2], s[3]));
      float e[U];
#pragma unroll
      for (int u = 0; u < U; ++u) e[u] = j0 + u * NSTREAM + stream < len ? __builtin_amdgcn_exp2f(s[u] - m_new) : 0.f;
      l[g] = l[g] * __builtin_amdgcn_exp2f(m[g] - m_new) + ((e[0] + e[1]) + (e[2] + e[3]));
      m[g] = m_new;
    }
  }
  if (dc == 0) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      sm_m[g][stream] = m[g];
      sm_l[g][stream] = l[g];
    }
  }
  __syncthreads();
  if (threadIdx.x < NG) {               // one thread per head folds the streams in stream order (a stream without a key: l = 0)
    const int g = threadIdx.x;
    float M = SM_NEG_BIG;
    for (int s = 0; s < NSTREAM; ++s) M = fmaxf(M, sm_m[g][s]);
    float L = 0.f;
    for (int s = 0; s < NSTREAM; ++s) L += sm_l[g][s] * __builtin_amdgcn_exp2f(sm_m[g][s] - M);
    sm_ML[g][0] = M;
    sm_ML[g][1] = L;
  }
  __syncthreads();
  float Mx[NG], Lx[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    Mx[g] = sm_ML[g][0];
    Lx[g] = sm_ML[g][1];
  }

  // ---- pass 2: the weights, and their segment sums a tile at a time
  float acc = 0.f;
  for (int j0 = 0; j0 < len; j0 += TK) {
    u32x4 kr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) kr[u] = *(const u32x4*)(kp + (int64_t)min(j0 + u * NSTREAM + stream, len - 1) * D);
    if (threadIdx.x < TK) {
      const int j = j0 + threadIdx.x;
      segt[threadIdx.x] = j < len ? (int)seg[(int64_t)b * ld_seg + j] : 255;
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float d = segmass_dot(q[g], kr[u]);
#pragma unroll
        for (int x = 1; x < LPR; x <<= 1) d += __shfl_xor(d, x, 64);
        const int j = j0 + u * NSTREAM + stream;
        const float p = j < len ? __builtin_amdgcn_exp2f(d - Mx[g]) / Lx[g] : 0.f;
        if (dc == 0) {
          pt[g][u * NSTREAM + stream] = p;
          if (probs != nullptr && j < len) probs[((int64_t)b * n_heads + (int64_t)h * NG + g) * ld_probs + j] = p;
        }
      }
    }
    __syncthreads();
    if (mass_thread) {
      const int cnt = min(TK, len - j0);
      for (int jj = 0; jj < cnt; ++jj) acc += segt[jj] == ms ? pt[mg][jj] : 0.f;
    }
    __syncthreads();                    // the next tile overwrites pt / segt
  }
  if (mass_thread) mrow[mg * n_seg + ms] = acc;
}

}  // namespace

extern "C" int icl_attn_segmass_bf16(const void* Q, int64_t ldq, const int32_t* q_rows, const void* Kc, const int32_t* lens,
                                     const uint8_t* seg, int64_t ld_seg, int32_t n_seg, float* mass, float* probs,
                                     int64_t ld_probs, int32_t n_seqs, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim,
                                     int32_t max_len, float scale, void* stream) {
  ICL_CHECK_ARG(Q != nullptr, "icl_attn_segmass_bf16: Q is NULL");
  ICL_CHECK_ARG(Kc != nullptr, "icl_attn_segmass_bf16: Kc is NULL");
  ICL_CHECK_ARG(lens != nullptr, "icl_attn_segmass_bf16: lens is NULL");
  ICL_CHECK_ARG(seg != nullptr, "icl_attn_segmass_bf16: seg is NULL");
  ICL_CHECK_ARG(mass != nullptr, "icl_attn_segmass_bf16: mass is NULL");
  ICL_CHECK_ARG(n_seg >= 1 && n_seg <= SM_MAX_SEG, "icl_attn_segmass_bf16: n_seg=%d (1..%d)", n_seg, SM_MAX_SEG);
  ICL_CHECK_ARG(head_dim == 64 || head_dim == 128, "icl_attn_segmass_bf16: head_dim=%d (only 64 and 128)", head_dim);
  ICL_CHECK_ARG(n_seqs > 0 && n_seqs <= 65535 && n_heads > 0 && max_len > 0,
                "icl_attn_segmass_bf16: bad sizes (n_seqs=%d, n_heads=%d, max_len=%d)", n_seqs, n_heads, max_len);
  if (n_kv_heads == 0) n_kv_heads = n_heads;
  ICL_CHECK_ARG(n_kv_heads > 0 && n_heads % n_kv_heads == 0,
                "icl_attn_segmass_bf16: n_heads=%d is not a multiple of n_kv_heads=%d", n_heads, n_kv_heads);
  const int group = n_heads / n_kv_heads;
  ICL_CHECK_ARG(group <= 8, "icl_attn_segmass_bf16: n_kv_heads=%d gives %d query heads per K/V head (at most 8)", n_kv_heads, group);
  ICL_CHECK_ARG(group == 1 || head_dim == 128,
                "icl_attn_segmass_bf16: n_kv_heads=%d with head_dim=%d (grouped-query attention: only 128)", n_kv_heads, head_dim);
  ICL_CHECK_ARG(ld_seg >= max_len, "icl_attn_segmass_bf16: ld_seg=%lld < max_len=%d", (long long)ld_seg, max_len);
  ICL_CHECK_ARG(probs == nullptr || ld_probs >= max_len, "icl_attn_segmass_bf16: ld_probs=%lld < max_len=%d", (long long)ld_probs,
                max_len);
  ICL_CHECK_ARG(__builtin_isfinite(scale),"icl_attn_segmass_bf16: scale is not finite");
  ICL_CHECK_ARG(ldq % 8 == 0 && ldq >= (int64_t)n_heads * head_dim && ((uintptr_t)Q & 15) == 0 && ((uintptr_t)Kc & 15) == 0 &&
                    ((uintptr_t)mass & 3) == 0 && ((uintptr_t)probs & 3) == 0,
                "icl_attn_segmass_bf16: misaligned operands (ldq must hold n_heads * head_dim columns, ldq %% 8 == 0)");
  dim3 grid(n_kv_heads, n_seqs);
#define ICL_SEGMASS_CASE(DD, GG)                                                                                               \
  hipLaunchKernelGGL((attn_segmass_kernel<DD, GG>), grid, dim3(256), 0, (hipStream_t)stream, (const unsigned short*)Q, ldq,   \
                     q_rows, (const unsigned short*)Kc, lens, seg, ld_seg, n_seg, mass, probs, ld_probs, n_kv_heads, max_len,  \
                     scale * SM_LOG2E)
  if (head_dim == 64) {
    ICL_SEGMASS_CASE(64, 1);
  } else {
    switch (group) {
      case 1: ICL_SEGMASS_CASE(128, 1); break;
      case 2: ICL_SEGMASS_CASE(128, 2); break;
      case 3: ICL_SEGMASS_CASE(128, 3); break;
      case 4: ICL_SEGMASS_CASE(128, 4); break;
      case 5: ICL_SEGMASS_CASE(128, 5); break;
      case 6: ICL_SEGMASS_CASE(128, 6); break;
      case 7: ICL_SEGMASS_CASE(128, 7); break;
      case 8: ICL_SEGMASS_CASE(128, 8); break;
    }
  }
#undef ICL_SEGMASS_CASE
  ICL_CHECK_LAUNCH("icl_attn_segmass_bf16");
  return ICL_OK;
}

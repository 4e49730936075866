// kv_fp8.hip — the FP8 KV cache's append and copy kernels (gfx950).  Layout and rounding: include/icl_hip.h, "FP8 KV cache".
// A cache row (sequence, head, position) is head_dim e4m3fn bytes; its f32 scale 2^e sits in a plane of its own, scale[seq][head][pos].
#include "common.h"

namespace {

// One block per qkv row m.  A head row (q, k or v of one head) is handled by LPR = D / 8 adjacent lanes, 8 elements each, so its
// maximum is a shuffle over the group (kv_fp8_quant8).  ROPE (icl_rope_kv_fp8): q and k are rotated at pos[m] with rope_rot8 (the
// bf16 rope_kv_kernel's function and rounding points), q in place, k only into the cache.  Without ROPE (icl_kv_append_fp8) k and
// v are taken as they are (the prefill QKV GEMM has rotated k in its epilogue).  A position outside [0, max_len) writes nothing.
template <int D, bool ROPE>
__global__ __launch_bounds__(256) void kv_fp8_append_kernel(unsigned short* qkv, int64_t ld, int64_t k_off, int64_t v_off,
                                                            const float* cosT, const float* sinT, const int* pos, const int* seq_ids,
                                                            unsigned char* kq, unsigned char* vq, float* ks, float* vs, int H,
                                                            int max_len) {
  constexpr int LPR = D / 8, HALF = D / 2, RPB = 256 / LPR;
  const int64_t m = blockIdx.x;
  const int p = pos[m];
  const bool store = p >= 0 && p < max_len;
  const int dc = threadIdx.x % LPR;
  const int64_t srow = (int64_t)seq_ids[m] * H;
  unsigned short* row = qkv + m * ld;
  const int n_items = (ROPE ? 3 : 2) * H;
  for (int it = threadIdx.x / LPR; it < n_items; it += RPB) {     // uniform over a lane group
    const int which = (ROPE ? 0 : 1) + it / H;                     // 0 = q, 1 = k, 2 = v
    const int h = it % H;
    unsigned short* bp = row + (which == 0 ? 0 : which == 1 ? k_off : v_off) + h * D;
    u32x4 x;
    if (ROPE && which < 2) {
      const int i0 = (dc % (LPR / 2)) * 8;                         // this lane's 8 elements of the low half (partner: + HALF)
      const u32x4 lo = *(const u32x4*)(bp + i0), hi = *(const u32x4*)(bp + i0 + HALF);
      const float* cp = cosT + (int64_t)p * HALF + i0;
      const float* sp = sinT + (int64_t)p * HALF + i0;
      u32x4 olo, ohi;
      rope_rot8(lo, hi, *(const f32x4*)cp, *(const f32x4*)(cp + 4), *(const f32x4*)sp, *(const f32x4*)(sp + 4), olo, ohi);
      x = dc >= LPR / 2 ? ohi : olo;
      if (which == 0) {            // every load of the row has been consumed above: the group's lanes rewrite their own chunks
        *(u32x4*)(bp + dc * 8) = x;
        continue;
      }
    } else {
      x = *(const u32x4*)(bp + dc * 8);
    }
    u32x2 q;
    float sc;
    kv_fp8_quant8<LPR>(x, q, sc);
    if (store) {
      const int64_t r = (srow + h) * max_len + p;
      *(u32x2*)((which == 1 ? kq : vq) + r * D + dc * 8) = q;
      if (dc == 0) (which == 1 ? ks : vs)[r] = sc;
    }
  }
}

// kv_copy_spans_kernel (beam.hip) for the two planes of an fp8 cache: 16 B of row bytes and then one scale per thread.
__global__ __launch_bounds__(256) void kv_copy_spans_fp8_kernel(
    const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, const float* __restrict__ ssrc, float* __restrict__ sdst,
    int64_t s_layer, int64_t s_seq, int64_t s_head, int64_t d_layer, int64_t d_seq, int64_t d_head, int64_t ss_layer, int64_t ss_seq,
    int64_t ss_head, int64_t sd_layer, int64_t sd_seq, int64_t sd_head, const int* __restrict__ src_seq,
    const int* __restrict__ src_t0, const int* __restrict__ dst_seq, const int* __restrict__ dst_t0, const int* __restrict__ n_t,
    int n_fixed, int H, int D, int src_n_seqs, int dst_n_seqs, int src_len, int dst_len) {
  const int r = blockIdx.x / H, h = blockIdx.x % H, l = blockIdx.y;
  // device-side ids and counts are clamped to the extents the caller described, as in kv_copy_spans_kernel
  const int ss = min(max(src_seq ? src_seq[r] : r, 0), src_n_seqs - 1);
  const int ds = min(max(dst_seq ? dst_seq[r] : r, 0), dst_n_seqs - 1);
  const int st0 = min(max(src_t0 ? src_t0[r] : 0, 0), src_len);
  const int dt0 = min(max(dst_t0 ? dst_t0[r] : 0, 0), dst_len);
  const int n = min(min(max(n_t ? n_t[r] : n_fixed, 0), src_len - st0), dst_len - dt0);
  const u32x4* sp = (const u32x4*)(src + l * s_layer + ss * s_seq + h * s_head + (int64_t)st0 * D);
  u32x4* dp = (u32x4*)(dst + l * d_layer + ds * d_seq + h * d_head + (int64_t)dt0 * D);
  const int chunks = n * D / 16;
  for (int i = threadIdx.x; i < chunks; i += 256) dp[i] = sp[i];
  const float* ssp = ssrc + l * ss_layer + ss * ss_seq + h * ss_head + st0;
  float* sdp = sdst + l * sd_layer + ds * sd_seq + h * sd_head + dt0;
  for (int i = threadIdx.x; i < n; i += 256) sdp[i] = ssp[i];
}

template <bool ROPE>
int launch_kv_fp8_append(void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const float* cosT, const float* sinT,
                         const int32_t* pos, const int32_t* seq_ids, void* kq, void* vq, float* ks, float* vs, int32_t M,
                         int32_t n_heads, int32_t head_dim, int32_t max_len, void* stream) {
#define ICL_KV_APPEND(DD)                                                                                                   \
  hipLaunchKernelGGL((kv_fp8_append_kernel<DD, ROPE>), dim3(M), dim3(256), 0, (hipStream_t)stream, (unsigned short*)qkv, ld, \
                     k_off, v_off, cosT, sinT, pos, seq_ids, (unsigned char*)kq, (unsigned char*)vq, ks, vs, n_heads, max_len)
  if (head_dim == 64) ICL_KV_APPEND(64); else ICL_KV_APPEND(128);
#undef ICL_KV_APPEND
  return ICL_OK;
}

}  // namespace

#define ICL_KV_FP8_COMMON_CHECKS(who)                                                                                        \
  ICL_CHECK_ARG(qkv && pos && seq_ids && kq && vq && kscale && vscale, who ": NULL pointer");                               \
  ICL_CHECK_ARG(M > 0 && n_heads > 0 && max_len > 0, who ": M, n_heads and max_len must be > 0");                           \
  ICL_CHECK_ARG(head_dim == 64 || head_dim == 128, who ": head_dim=%d (only 64 and 128)", head_dim);                        \
  ICL_CHECK_ARG(ld % 8 == 0 && k_off % 8 == 0 && v_off % 8 == 0 && ((uintptr_t)qkv & 15) == 0,                              \
                who ": qkv must be 16-byte aligned with ld/k_off/v_off multiples of 8");                                     \
  ICL_CHECK_ARG(k_off >= (int64_t)n_heads * head_dim && v_off >= k_off + (int64_t)n_heads * head_dim &&                      \
                    ld >= v_off + (int64_t)n_heads * head_dim,                                                               \
                who ": q | k | v column blocks must be disjoint inside a row");                                              \
  ICL_CHECK_ARG(((uintptr_t)kq & 15) == 0 && ((uintptr_t)vq & 15) == 0 && ((uintptr_t)kscale & 3) == 0 &&                    \
                    ((uintptr_t)vscale & 3) == 0, who ": cache misaligned")

extern "C" int icl_rope_kv_fp8(void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const float* cosT, const float* sinT,
                               const int32_t* pos, const int32_t* seq_ids, void* kq, void* vq, float* kscale, float* vscale,
                               int32_t M, int32_t n_heads, int32_t head_dim, int32_t max_len, void* stream) {
  ICL_KV_FP8_COMMON_CHECKS("icl_rope_kv_fp8");
  ICL_CHECK_ARG(cosT && sinT && ((uintptr_t)cosT & 15) == 0 && ((uintptr_t)sinT & 15) == 0, "icl_rope_kv_fp8: cos/sin NULL or misaligned");
  launch_kv_fp8_append<true>(qkv, ld, k_off, v_off, cosT, sinT, pos, seq_ids, kq, vq, kscale, vscale, M, n_heads, head_dim, max_len,
                             stream);
  ICL_CHECK_LAUNCH("icl_rope_kv_fp8");
  return ICL_OK;
}

extern "C" int icl_kv_append_fp8(const void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const int32_t* pos, const int32_t* seq_ids,
                                 void* kq, void* vq, float* kscale, float* vscale, int32_t M, int32_t n_heads, int32_t head_dim,
                                 int32_t max_len, void* stream) {
  ICL_KV_FP8_COMMON_CHECKS("icl_kv_append_fp8");
  launch_kv_fp8_append<false>((void*)qkv, ld, k_off, v_off, nullptr, nullptr, pos, seq_ids, kq, vq, kscale, vscale, M, n_heads,
                              head_dim, max_len, stream);
  ICL_CHECK_LAUNCH("icl_kv_append_fp8");
  return ICL_OK;
}
#undef ICL_KV_FP8_COMMON_CHECKS

extern "C" int icl_kv_copy_spans_fp8(const void* src, const float* src_scale, void* dst, float* dst_scale, int64_t src_layer_stride,
                                     int64_t src_seq_stride, int64_t src_head_stride, int64_t dst_layer_stride, int64_t dst_seq_stride,
                                     int64_t dst_head_stride, int64_t src_scale_layer_stride, int64_t src_scale_seq_stride,
                                     int64_t src_scale_head_stride, int64_t dst_scale_layer_stride, int64_t dst_scale_seq_stride,
                                     int64_t dst_scale_head_stride, const int32_t* src_seq, const int32_t* src_t0,
                                     const int32_t* dst_seq, const int32_t* dst_t0, const int32_t* n_t, int32_t n_fixed, int32_t n_rows,
                                     int32_t n_layers, int32_t n_heads, int32_t head_dim, int32_t src_n_seqs, int32_t dst_n_seqs,
                                     int32_t src_len, int32_t dst_len, void* stream) {
  ICL_CHECK_ARG(src && dst && src_scale && dst_scale, "icl_kv_copy_spans_fp8: NULL pointer");
  ICL_CHECK_ARG(src_n_seqs > 0 && dst_n_seqs > 0 && src_len > 0 && dst_len > 0,
                "icl_kv_copy_spans_fp8: src / dst extents (sequences, positions) must be > 0");
  ICL_CHECK_ARG((src_seq || n_rows <= src_n_seqs) && (dst_seq || n_rows <= dst_n_seqs),
                "icl_kv_copy_spans_fp8: n_rows=%d exceeds the %d / %d sequences of src / dst", n_rows, src_n_seqs, dst_n_seqs);
  ICL_CHECK_ARG(n_rows > 0 && n_layers > 0 && n_heads > 0 && head_dim > 0 && head_dim % 16 == 0,
                "icl_kv_copy_spans_fp8: bad sizes (head_dim must be a multiple of 16)");
  ICL_CHECK_ARG(n_t || n_fixed >= 0, "icl_kv_copy_spans_fp8: n_fixed < 0");
  ICL_CHECK_ARG(((uintptr_t)src | (uintptr_t)dst) % 16 == 0 &&
                    (src_layer_stride | src_seq_stride | src_head_stride | dst_layer_stride | dst_seq_stride | dst_head_stride) % 16 == 0,
                "icl_kv_copy_spans_fp8: byte planes and their strides must be 16-byte aligned");
  ICL_CHECK_ARG(((uintptr_t)src_scale | (uintptr_t)dst_scale) % 4 == 0, "icl_kv_copy_spans_fp8: scale planes misaligned");
  ICL_CHECK_ARG((int64_t)n_rows * n_heads < 0x7fffffffLL && n_layers <= 65535, "icl_kv_copy_spans_fp8: grid too large");
  if (!n_t && n_fixed == 0) return ICL_OK;
  hipLaunchKernelGGL(kv_copy_spans_fp8_kernel, dim3(n_rows * n_heads, n_layers), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)src, (unsigned char*)dst, src_scale, dst_scale, src_layer_stride, src_seq_stride,
                     src_head_stride, dst_layer_stride, dst_seq_stride, dst_head_stride, src_scale_layer_stride, src_scale_seq_stride,
                     src_scale_head_stride, dst_scale_layer_stride, dst_scale_seq_stride, dst_scale_head_stride, src_seq, src_t0,
                     dst_seq, dst_t0, n_t, n_fixed, n_heads, head_dim, src_n_seqs, dst_n_seqs, src_len, dst_len);
  ICL_CHECK_LAUNCH("icl_kv_copy_spans_fp8");
  return ICL_OK;
}

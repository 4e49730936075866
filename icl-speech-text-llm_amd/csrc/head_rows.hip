// head_rows.hip — capture and patch of single attention heads' outputs at listed rows of the bf16 attention-output buffer, the
// operand of o_proj (gfx950).  Contract and numerics: include/icl_hip.h (icl_head_rows_bf16).
//
// head_rows_kernel<CAP, PATCH>: blockIdx.x = list entry r (row = rows[r]), blockIdx.y * 256 + threadIdx.x = one 16-byte chunk (8
// bf16) of the row: a head row of D elements sits on D/8 adjacent lanes.  With a capture the chunks are those of all n_heads
// heads (the thread of head h looks h up in heads[] — a uniform scan of n_sel <= n_heads entries — and patches its chunk when it
// is selected, so the capture and the patch of an element are the same thread's and the capture is pre-patch without a
// barrier); without one they are those of the n_sel selected heads only.  A thread works on ONE chunk: its loads (heads[], the
// att chunk, the two 16-byte halves of its 8 vector floats) are all issued before its first store (the capture chunk, then the
// att chunk), the pattern of resid_rows_kernel and rope_kv_rows_kernel; the replace-only form never loads att.  Capture moves
// u32x4 bits (NaN payloads, -0.0 and subnormals survive); replace is f32_to_bf16_bits (RNE; round_bf16) per element, add one __fmaf_rn per
// element on the widened bf16 and then that rounding.  Every address is an int64_t product of the entry, the row, the head and a
// leading dimension.  No LDS, no atomics, no cross-lane traffic; a row listed twice or a head selected twice is the caller's
// error.  The grid depends on the list's length only through blockIdx.x, and no thread's arithmetic depends on the grid: a row's
// bits cannot depend on the list it travels in.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), no scratch and no LDS in any of them:
//     <CAP, PATCH>                     VGPRs  SGPRs  waves per SIMD
//     <1, 0>  capture                      6    20     8
//     <0, 1>  replace                     21    24     8
//     <1, 1>  capture + replace           21    26     8
//     <0, 2>  add                         18    26     8
//     <1, 2>  capture + add               24    26     8
#include <math.h>
#include "common.h"

namespace {

enum : int { PATCH_NONE = 0, PATCH_REPLACE = 1, PATCH_ADD = 2 };

// f32_to_bf16_bits; with BITS a value whose low half is zero — a bf16 value — is handed through as its upper half, so that a
// replace returns such a vector's bits whatever the conversion instruction does to a NaN's payload (for every other value of
// that kind the two agree)
template <bool BITS>
__device__ __forceinline__ unsigned short round_bf16(float f) {
  const unsigned int b = __float_as_uint(f);
  return BITS && (b & 0xffffu) == 0 ? (unsigned short)(b >> 16) : f32_to_bf16_bits(f);
}

template <bool CAP, int PATCH>
__global__ __launch_bounds__(256) void head_rows_kernel(unsigned short* att, int64_t ld_att, const int* rows, int n_heads, int head_dim,
                                                        unsigned short* capture, int64_t ld_cap, const int* heads, int n_sel,
                                                        const float* vec, int64_t ld_vec, float alpha) {
  const int64_t r = blockIdx.x;
  const int per = head_dim >> 3;                                   // 16-byte chunks of a head row: 8 or 16
  const int u = blockIdx.y * 256 + threadIdx.x;                    // the chunk among those of the heads this form walks
  const int first = u / per, j = u - first * per;
  if (first >= (CAP ? n_heads : n_sel)) return;
  int h = first, s = PATCH != PATCH_NONE && !CAP ? first : -1;     // the head, and its place in heads[] (-1: not selected)
  if constexpr (PATCH != PATCH_NONE) {
    if constexpr (CAP) {
      for (int t = 0; t < n_sel; ++t) s = heads[t] == h ? t : s;
    } else {
      h = heads[first];
    }
  }
  const int64_t col = (int64_t)h * head_dim + (int64_t)j * 8;
  unsigned short* ap = att + (int64_t)rows[r] * ld_att + col;
  u32x4 x = {}, v0 = {}, v1 = {};
  if constexpr (CAP || PATCH == PATCH_ADD) x = *(const u32x4*)ap;
  if constexpr (PATCH != PATCH_NONE) {
    if (s >= 0) {
      const float* vp = vec + r * ld_vec + (int64_t)s * head_dim + (int64_t)j * 8;      // ld_vec == 0: one block of vectors for every entry
      v0 = *(const u32x4*)vp;
      v1 = *(const u32x4*)(vp + 4);
    }
  }
  if constexpr (CAP) *(u32x4*)(capture + r * ld_cap + col) = x;    // always the pre-patch value
  if constexpr (PATCH != PATCH_NONE) {
    if (s >= 0) {
      u32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float lo = __uint_as_float(k < 2 ? v0[2 * k] : v1[2 * k - 4]), hi = __uint_as_float(k < 2 ? v0[2 * k + 1] : v1[2 * k - 3]);
        if constexpr (PATCH == PATCH_ADD) {
          lo = __fmaf_rn(alpha, lo, bf16_bits_to_f32((unsigned short)(x[k] & 0xffffu)));
          hi = __fmaf_rn(alpha, hi, bf16_bits_to_f32((unsigned short)(x[k] >> 16)));
        }
        o[k] = (unsigned int)round_bf16<PATCH == PATCH_REPLACE>(lo) | ((unsigned int)round_bf16<PATCH == PATCH_REPLACE>(hi) << 16);
      }
      *(u32x4*)ap = o;
    }
  }
}

template <bool CAP, int PATCH>
void head_rows_launch(void* att, int64_t ld_att, const int32_t* rows, int32_t n_rows, int32_t n_heads, int32_t head_dim, void* capture,
                      int64_t ld_cap, const int32_t* heads, int32_t n_sel, const float* vec, int64_t ld_vec, float alpha, void* stream) {
  const int chunks = (CAP ? n_heads : n_sel) * (head_dim / 8);
  hipLaunchKernelGGL((head_rows_kernel<CAP, PATCH>), dim3(n_rows, (chunks + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     (unsigned short*)att, ld_att, rows, n_heads, head_dim, (unsigned short*)capture, ld_cap, heads, n_sel, vec, ld_vec, alpha);
}

}  // namespace

extern "C" int icl_head_rows_bf16(void* att, int64_t ld_att, const int32_t* rows, int32_t n_rows, int32_t n_heads, int32_t head_dim,
                                  void* capture, int64_t ld_cap, const int32_t* heads, int32_t n_sel, const float* vec,
                                  int64_t ld_vec, int32_t mode, float alpha, void* stream) {
  const char* who = "icl_head_rows_bf16";
  const auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  ICL_CHECK_ARG(att != nullptr, "%s: att is NULL", who);
  ICL_CHECK_ARG(rows != nullptr, "%s: rows is NULL", who);
  ICL_CHECK_ARG(capture != nullptr || vec != nullptr, "%s: capture and vec are both NULL (nothing to do)", who);
  ICL_CHECK_ARG(vec == nullptr || heads != nullptr, "%s: heads is NULL with vec given", who);
  ICL_CHECK_ARG(n_rows >= 1 && n_rows <= 65535, "%s: n_rows=%d must be in 1..65535", who, n_rows);
  ICL_CHECK_ARG(head_dim == 64 || head_dim == 128, "%s: head_dim=%d must be 64 or 128", who, head_dim);
  ICL_CHECK_ARG(n_heads >= 1 && n_heads <= 65535, "%s: n_heads=%d must be in 1..65535", who, n_heads);
  if (vec) ICL_CHECK_ARG(n_sel >= 1 && n_sel <= n_heads, "%s: n_sel=%d must be in 1..n_heads=%d", who, n_sel, n_heads);
  const int64_t width = (int64_t)n_heads * head_dim;
  ICL_CHECK_ARG(ld_att >= width && ld_att % 8 == 0, "%s: ld_att=%lld must be a multiple of 8, at least n_heads*head_dim", who, (long long)ld_att);
  if (capture) ICL_CHECK_ARG(ld_cap >= width && ld_cap % 8 == 0, "%s: ld_cap=%lld must be a multiple of 8, at least n_heads*head_dim", who, (long long)ld_cap);
  if (vec) ICL_CHECK_ARG(ld_vec == 0 || (ld_vec >= (int64_t)n_sel * head_dim && ld_vec % 4 == 0),
                         "%s: ld_vec=%lld must be 0 or a multiple of 4, at least n_sel*head_dim", who, (long long)ld_vec);
  ICL_CHECK_ARG(al16(att), "%s: att is not 16-byte aligned", who);
  ICL_CHECK_ARG(((uintptr_t)rows & 3) == 0 && ((uintptr_t)heads & 3) == 0, "%s: rows or heads is not 4-byte aligned", who);
  ICL_CHECK_ARG(al16(capture), "%s: capture is not 16-byte aligned", who);
  ICL_CHECK_ARG(al16(vec), "%s: vec is not 16-byte aligned", who);
  ICL_CHECK_ARG(mode == 0 || mode == 1, "%s: mode=%d must be 0 (replace) or 1 (add)", who, mode);
  ICL_CHECK_ARG(isfinite(alpha), "%s: alpha must be finite", who);
#define HEAD_ARGS att, ld_att, rows, n_rows, n_heads, head_dim, capture, ld_cap, heads, n_sel, vec, ld_vec, alpha, stream
  if (!vec) head_rows_launch<true, PATCH_NONE>(HEAD_ARGS);
  else if (mode == 0) capture ? head_rows_launch<true, PATCH_REPLACE>(HEAD_ARGS) : head_rows_launch<false, PATCH_REPLACE>(HEAD_ARGS);
  else capture ? head_rows_launch<true, PATCH_ADD>(HEAD_ARGS) : head_rows_launch<false, PATCH_ADD>(HEAD_ARGS);
#undef HEAD_ARGS
  ICL_CHECK_LAUNCH(who);
  return ICL_OK;
}

// resid_rows.hip — capture and patch of listed rows of the f32 residual stream (gfx950).  Contract and numerics:
// include/icl_hip.h (icl_resid_rows_f32).
//
// resid_rows_kernel<CAP, PATCH>: one block per list entry r, 256 threads, row = rows[r].  A pass is 256 chunks of 16 B (1024
// elements): thread t works on elements 4 t .. 4 t + 3 of the pass.  All of a pass's loads (the h chunk, the vector chunk) are
// issued before its first store (the capture chunk, then the h chunk), the pattern of rope_kv_rows_kernel; the replace-only form
// never loads h.  Capture and replace move u32x4 bits (NaN payloads, -0.0 and subnormals survive); add is one __fmaf_rn per
// element on the f32 values.  Every address is an int64_t product of the entry, the row and a leading dimension.  No LDS, no
// atomics, no cross-lane traffic; a row listed twice is the caller's error (two blocks would race on it).
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), no scratch and no LDS in any of them:
//     <CAP, PATCH>                     VGPRs  SGPRs  waves per SIMD
//     <1, 0>  capture                     10    22     8
//     <0, 1>  replace                     10    22     8
//     <1, 1>  capture + replace           16    26     8
//     <0, 2>  add                         14    25     8
//     <1, 2>  capture + add               16    29     8
#include <math.h>
#include "common.h"

namespace {

enum : int { PATCH_NONE = 0, PATCH_REPLACE = 1, PATCH_ADD = 2 };

template <bool CAP, int PATCH>
__global__ __launch_bounds__(256) void resid_rows_kernel(float* h, int64_t ldh, const int* rows, int hidden, float* capture,
                                                         int64_t ld_cap, const float* vec, int64_t ld_vec, float alpha) {
  const int64_t r = blockIdx.x;
  float* hp = h + (int64_t)rows[r] * ldh;
  float* cp = CAP ? capture + r * ld_cap : nullptr;
  const float* vp = PATCH != PATCH_NONE ? vec + r * ld_vec : nullptr;      // ld_vec == 0: one vector for every entry
  for (int64_t i = (int64_t)threadIdx.x * 4; i < hidden; i += 1024) {
    u32x4 x = {}, v = {};
    if constexpr (CAP || PATCH == PATCH_ADD) x = *(const u32x4*)(hp + i);
    if constexpr (PATCH != PATCH_NONE) v = *(const u32x4*)(vp + i);
    if constexpr (CAP) *(u32x4*)(cp + i) = x;                             // always the pre-patch value
    if constexpr (PATCH == PATCH_REPLACE) *(u32x4*)(hp + i) = v;
    if constexpr (PATCH == PATCH_ADD) {
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = __float_as_uint(__fmaf_rn(alpha, __uint_as_float(v[j]), __uint_as_float(x[j])));
      *(u32x4*)(hp + i) = o;
    }
  }
}

template <bool CAP, int PATCH>
void resid_rows_launch(float* h, int64_t ldh, const int32_t* rows, int32_t n_rows, int32_t hidden, float* capture, int64_t ld_cap,
                       const float* vec, int64_t ld_vec, float alpha, void* stream) {
  hipLaunchKernelGGL((resid_rows_kernel<CAP, PATCH>), dim3(n_rows), dim3(256), 0, (hipStream_t)stream, h, ldh, rows, hidden, capture,
                     ld_cap, vec, ld_vec, alpha);
}

}  // namespace

extern "C" int icl_resid_rows_f32(float* h, int64_t ldh, const int32_t* rows, int32_t n_rows, int32_t hidden, float* capture,
                                  int64_t ld_cap, const float* vec, int64_t ld_vec, int32_t mode, float alpha, void* stream) {
  const char* who = "icl_resid_rows_f32";
  const auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  ICL_CHECK_ARG(h != nullptr, "%s: h is NULL", who);
  ICL_CHECK_ARG(rows != nullptr, "%s: rows is NULL", who);
  ICL_CHECK_ARG(capture != nullptr || vec != nullptr, "%s: capture and vec are both NULL (nothing to do)", who);
  ICL_CHECK_ARG(n_rows >= 1 && n_rows <= 65535, "%s: n_rows=%d must be in 1..65535", who, n_rows);
  ICL_CHECK_ARG(hidden > 0 && hidden % 4 == 0, "%s: hidden=%d must be a positive multiple of 4", who, hidden);
  ICL_CHECK_ARG(ldh >= hidden && ldh % 4 == 0, "%s: ldh=%lld must be a multiple of 4, at least hidden", who, (long long)ldh);
  if (capture) ICL_CHECK_ARG(ld_cap >= hidden && ld_cap % 4 == 0, "%s: ld_cap=%lld must be a multiple of 4, at least hidden", who, (long long)ld_cap);
  if (vec) ICL_CHECK_ARG(ld_vec == 0 || (ld_vec >= hidden && ld_vec % 4 == 0), "%s: ld_vec=%lld must be 0 or a multiple of 4, at least hidden", who, (long long)ld_vec);
  ICL_CHECK_ARG(al16(h), "%s: h is not 16-byte aligned", who);
  ICL_CHECK_ARG(((uintptr_t)rows & 3) == 0, "%s: rows is not 4-byte aligned", who);
  ICL_CHECK_ARG(al16(capture), "%s: capture is not 16-byte aligned", who);
  ICL_CHECK_ARG(al16(vec), "%s: vec is not 16-byte aligned", who);
  ICL_CHECK_ARG(mode == 0 || mode == 1, "%s: mode=%d must be 0 (replace) or 1 (add)", who, mode);
  ICL_CHECK_ARG(isfinite(alpha), "%s: alpha must be finite", who);
#define RESID_ARGS h, ldh, rows, n_rows, hidden, capture, ld_cap, vec, ld_vec, alpha, stream
  if (!vec) resid_rows_launch<true, PATCH_NONE>(RESID_ARGS);
  else if (mode == 0) capture ? resid_rows_launch<true, PATCH_REPLACE>(RESID_ARGS) : resid_rows_launch<false, PATCH_REPLACE>(RESID_ARGS);
  else capture ? resid_rows_launch<true, PATCH_ADD>(RESID_ARGS) : resid_rows_launch<false, PATCH_ADD>(RESID_ARGS);
#undef RESID_ARGS
  ICL_CHECK_LAUNCH(who);
  return ICL_OK;
}

// common.h — shared device/host helpers for libicl_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/icl_hip.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(8))) unsigned int u32x8;

// ---- error plumbing (host) ------------------------------------------------------------------
void icl_set_error(const char* fmt, ...);
#define ICL_CHECK_ARG(cond, ...)            \
  do {                                      \
    if (!(cond)) {                          \
      icl_set_error(__VA_ARGS__);           \
      return ICL_EINVAL;                    \
    }                                       \
  } while (0)
#define ICL_CHECK_LAUNCH(name)                                                      \
  do {                                                                              \
    hipError_t e__ = hipGetLastError();                                             \
    if (e__ != hipSuccess) {                                                        \
      icl_set_error("%s: launch failed: %s", name, hipGetErrorString(e__));         \
      return ICL_ELAUNCH;                                                           \
    }                                                                               \
  } while (0)

// ---- device helpers ---------------------------------------------------------------------------
__device__ __forceinline__ float bf16_bits_to_f32(unsigned short b) {
  return __uint_as_float(((unsigned int)b) << 16);
}
__device__ __forceinline__ unsigned short f32_to_bf16_bits(float f) {
  // plain cast: hipcc emits v_cvt_pk_bf16_f32 (RNE, NaN-preserving) on gfx950
  __bf16 h = (__bf16)f;
  return __builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ unsigned int pack_bf16x2(float lo, float hi) {
  bf16x2 v;
  v[0] = (__bf16)lo;
  v[1] = (__bf16)hi;
  return __builtin_bit_cast(unsigned int, v);
}
// RoPE on eight (i, i + D/2) pairs of one head (HF rotate_half pairing): lo/hi hold 8 bf16 each, c0|c1 and s0|s1 the eight
// f32 cos/sin values of those columns.  Products and sums are rounded separately (no FMA contraction) — the arithmetic of
// the f32 oracle — and the function is shared by the rope kernel and the fused QKV-GEMM epilogue so that both round alike.
__device__ __forceinline__ void rope_rot8(u32x4 lo, u32x4 hi, f32x4 c0, f32x4 c1, f32x4 s0, f32x4 s1, u32x4& olo,
                                          u32x4& ohi) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a0 = __uint_as_float(lo[j] << 16), a1 = __uint_as_float(lo[j] & 0xffff0000u);
    const float b0 = __uint_as_float(hi[j] << 16), b1 = __uint_as_float(hi[j] & 0xffff0000u);
    const float cA = j < 2 ? c0[2 * j] : c1[2 * j - 4], cB = j < 2 ? c0[2 * j + 1] : c1[2 * j - 3];
    const float sA = j < 2 ? s0[2 * j] : s1[2 * j - 4], sB = j < 2 ? s0[2 * j + 1] : s1[2 * j - 3];
    olo[j] = pack_bf16x2(__fsub_rn(__fmul_rn(a0, cA), __fmul_rn(b0, sA)), __fsub_rn(__fmul_rn(a1, cB), __fmul_rn(b1, sB)));
    ohi[j] = pack_bf16x2(__fadd_rn(__fmul_rn(b0, cA), __fmul_rn(a0, sA)), __fadd_rn(__fmul_rn(b1, cB), __fmul_rn(a1, sB)));
  }
}
// FP8 rounding rule shared by the weight packer (gemm_decode.hip) and the FP8 KV cache (rope_kv.hip, attn_decode.hip): the smallest e with
// m <= 448 * 2^e (0 for m = 0), and RNE into OCP e4m3fn of a value |x| <= 448.
__device__ __forceinline__ int fp8_row_exponent(float m) {
  if (m == 0.f) return 0;
  int k;
  const float f = frexpf(m, &k);            // m = f * 2^k, f in [0.5, 1);  448 = 0.875 * 2^9
  return f <= 0.875f ? k - 9 : k - 8;
}
// |x| <= 448: round to nearest even into e4m3fn, integer arithmetic on the f32 bits (sign kept, -0 -> 0x80 as torch does)
__device__ __forceinline__ unsigned f32_to_e4m3fn(float x) {
  const unsigned u = __float_as_uint(x), a = u & 0x7fffffffu;
  unsigned c;
  if (a < 0x3c800000u) c = (unsigned)rintf(__uint_as_float(a) * 512.f);   // |x| < 2^-6: the subnormal grid 2^-9 (8 -> 0x08 = 2^-6)
  else c = ((a + 0x7ffffu + ((a >> 20) & 1u)) >> 20) - (120u << 3);      // 3 mantissa bits, exponent bias 127 -> 7
  return ((u >> 24) & 0x80u) | c;
}
// FP8 KV cache (include/icl_hip.h, "FP8 KV cache"): one lane's 2*NW elements (NW dwords of bf16 pairs, element 2t in the low half
// of x[t]) of a head_dim row held by LPR adjacent lanes (all LPR lanes must call it) -> their e4m3fn codes (element i in byte i of
// q, NW/2 dwords) and the row scale 2^e.  A row with a non-finite element gets codes 0x7f (NaN) and a NaN scale: every element of it
// dequantizes to NaN.
template <int LPR, int NW>
__device__ __forceinline__ void kv_fp8_quant(const unsigned* x, unsigned* q, float& sc) {
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    const float x0 = fabsf(__uint_as_float(x[j] << 16)), x1 = fabsf(__uint_as_float(x[j] & 0xffff0000u));
    a = fmaxf(a, fmaxf(x0 <= 3.4028235e38f ? x0 : __builtin_inff(), x1 <= 3.4028235e38f ? x1 : __builtin_inff()));
  }
#pragma unroll
  for (int o = 1; o < LPR; o <<= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
  if (!(a <= 3.4028235e38f)) {
#pragma unroll
    for (int j = 0; j < NW / 2; ++j) q[j] = 0x7f7f7f7fu;
    sc = __uint_as_float(0x7fc00000u);
    return;
  }
  const int e = fp8_row_exponent(a);
  sc = ldexpf(1.f, e);
#pragma unroll
  for (int j = 0; j < NW / 2; ++j) q[j] = 0u;
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    const unsigned c0 = f32_to_e4m3fn(ldexpf(__uint_as_float(x[j] << 16), -e));
    const unsigned c1 = f32_to_e4m3fn(ldexpf(__uint_as_float(x[j] & 0xffff0000u), -e));
    q[j >> 1] |= (c0 | (c1 << 8)) << ((j & 1) * 16);
  }
}
template <int LPR>
__device__ __forceinline__ void kv_fp8_quant8(u32x4 x, u32x2& q, float& sc) {
  const unsigned xs[4] = {x[0], x[1], x[2], x[3]};
  unsigned qs[2];
  kv_fp8_quant<LPR, 4>(xs, qs, sc);
  q = u32x2{qs[0], qs[1]};
}
// 4 * NQ e4m3fn codes (element i in byte i) of a row with scale sc -> f32 q * sc (exact: x' of the contract)
template <int NQ>
__device__ __forceinline__ void kv_fp8_deq(const unsigned* q, float sc, float* out) {
  const f32x2 s = {sc, sc};
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(q[j], false) * s, b = __builtin_amdgcn_cvt_pk_f32_fp8(q[j], true) * s;
    out[4 * j] = a[0]; out[4 * j + 1] = a[1]; out[4 * j + 2] = b[0]; out[4 * j + 3] = b[1];
  }
}
// exact-erf GELU for the GEMM epilogues (128 values per thread, VALU-bound next to a K = 1280 main loop):
//     gelu(x) = x Phi(x) = relu(x) - |x| Q(|x|),   Q(t) = 1 - Phi(t) = erfc(t / sqrt 2) / 2 = 2^P(t)
// with P = log2 Q as ONE degree-7 polynomial (the -t^2/2 log2 e of the Gaussian tail folded into its quadratic term; minimax fit of
// log2(erfcx(t / sqrt 2) / 2) on [0, 7]: |dP| <= 1.4e-5, i.e. Q to 1e-5 RELATIVE everywhere; t is clamped to 7, where |x| Q < 1e-11).
// |gelu - exact| <= 1.5e-6 absolute and <= 1.3e-5 relative (tools/ checked over [-20, 20] in f32 arithmetic): two orders below a
// bf16 rounding of the result.  Per value pair: |x|, clamp, seven packed FMAs, two v_exp_f32, relu, one packed FMA — the
// Abramowitz-Stegun 7.1.26 form it replaces (rounds 1-3) needed a v_rcp_f32 per value on top (76 vs 108 issue cycles per pair) and
// carried a mistyped leading coefficient (0.53060 for 0.53070: 2.6e-5 absolute error, still far inside the tolerance, found when
// this form was checked against it).  Explicit FMAs only (the same contraction at every call site: all tile shapes must
// round alike), written on pairs so that hipcc emits v_pk_fma_f32 (two values per issue slot).
__device__ __forceinline__ f32x2 gelu_erf2(f32x2 x) {
  const f32x2 ax = __builtin_elementwise_abs(x);
  const f32x2 t = __builtin_elementwise_min(ax, f32x2{7.0f, 7.0f});
  f32x2 p = {-1.5882353683e-06f, -1.5882353683e-06f};
  p = __builtin_elementwise_fma(p, t, f32x2{5.6153733911e-05f, 5.6153733911e-05f});
  p = __builtin_elementwise_fma(p, t, f32x2{-8.8321799332e-04f, -8.8321799332e-04f});
  p = __builtin_elementwise_fma(p, t, f32x2{8.3032251061e-03f, 8.3032251061e-03f});
  p = __builtin_elementwise_fma(p, t, f32x2{-5.3501311510e-02f, -5.3501311510e-02f});
  p = __builtin_elementwise_fma(p, t, f32x2{-4.5896438201e-01f, -4.5896438201e-01f});
  p = __builtin_elementwise_fma(p, t, f32x2{-1.1510356065e+00f, -1.1510356065e+00f});
  p = __builtin_elementwise_fma(p, t, f32x2{-1.0000140186e+00f, -1.0000140186e+00f});
  const f32x2 q = {__builtin_amdgcn_exp2f(p[0]), __builtin_amdgcn_exp2f(p[1])};
  const f32x2 relu = __builtin_elementwise_max(x, f32x2{0.0f, 0.0f});
  return __builtin_elementwise_fma(-ax, q, relu);
}
__device__ __forceinline__ f32x4 gelu_erf4(f32x4 v) {
  const f32x2 a = gelu_erf2(f32x2{v[0], v[1]}), b = gelu_erf2(f32x2{v[2], v[3]});
  return f32x4{a[0], a[1], b[0], b[1]};
}
__device__ __forceinline__ float gelu_erf(float x) { return gelu_erf2(f32x2{x, x})[0]; }
__device__ __forceinline__ float silu_f(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }   // no IEEE division sequence

__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_reduce_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_reduce_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

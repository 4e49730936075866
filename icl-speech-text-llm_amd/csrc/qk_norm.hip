// qk_norm.hip — per-head q / k RMSNorm + RoPE + KV-cache append in one pass (gfx950), for decoders that normalise every q and
// k head over head_dim between the projection and the rotation (Qwen3).  Contract and numerics: include/icl_hip.h,
// icl_qknorm_rope_kv_bf16.
//
// One block per qkv row m, as rope_kv_kernel and kv_fp8_append_kernel.  A head row (q, k or v of one head) is held by LPR = D / 8
// adjacent lanes, lane dc its elements 8 dc .. 8 dc + 7 (one 16-B load), so a block works on 256 / LPR head rows at a time and
// U = 2 of them per thread per pass: 32 head rows a pass at head_dim 128, 64 at head_dim 64.  All of a pass's loads are issued
// before the first use; cos / sin and the two gamma chunks depend on the lane alone and are loaded once per block.
//
// Sum of squares, the documented order: a lane adds the squares of its eight elements in element order, s = 0, s += x[j]^2 for
// j = 0 .. 7 (a bf16 square is exact in f32, so the fused and the separate form of that step are the same number); the LPR
// partial sums are then folded by an xor butterfly over lane distances 1, 2, .. LPR / 2, so every lane of the group holds the
// same ss.  r = rsqrtf(ss * (1 / D) + eps);  n[i] = bf16_rne((x[i] * r) * gamma[i]).  The rotation needs element i and
// i + D / 2: lane dc takes its partner's n from lane dc ^ (LPR / 2) by shuffle, both run rope_rot8 on the same eight pairs and
// each keeps the half it owns — the function and the bf16 rounding points of rope_kv_kernel on a buffer holding n.
// v rows go to the cache as they are.  No LDS.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): 68 VGPRs and 46 SGPRs for both
// instantiations, no scratch, no LDS, occupancy 7 waves per SIMD.
#include "common.h"

namespace {

template <int D>
__global__ __launch_bounds__(256) void qknorm_rope_kv_kernel(unsigned short* qkv, int64_t ld, int64_t k_off, int64_t v_off,
                                                             const float* q_gamma, const float* k_gamma, float eps,
                                                             const float* cosT, const float* sinT, const int* pos,
                                                             const int* seq_ids, unsigned short* kc, unsigned short* vc, int H,
                                                             int Hkv, int max_len) {
  constexpr int LPR = D / 8, HALF = D / 2, RPB = 256 / LPR, U = 2;
  const int64_t m = blockIdx.x;
  const int p = pos[m];
  const int dc = threadIdx.x % LPR;
  const bool upper = dc >= LPR / 2;                       // this lane owns elements of the second half of the head row
  const int i0 = (dc % (LPR / 2)) * 8;                    // the eight (i, i + HALF) pairs this lane rotates
  unsigned short* row = qkv + m * ld;
  const int64_t cache_row = kc ? ((int64_t)seq_ids[m] * Hkv) * max_len + p : 0;
  const int n_rope = H + Hkv;                             // head rows: q heads, k heads, then (with a cache) v heads
  const int n_items = n_rope + (vc ? Hkv : 0);
  const float* cp = cosT + (int64_t)p * HALF + i0;
  const float* sp = sinT + (int64_t)p * HALF + i0;
  const f32x4 c0 = *(const f32x4*)cp, c1 = *(const f32x4*)(cp + 4), s0 = *(const f32x4*)sp, s1 = *(const f32x4*)(sp + 4);
  const f32x4 gq0 = *(const f32x4*)(q_gamma + dc * 8), gq1 = *(const f32x4*)(q_gamma + dc * 8 + 4);
  const f32x4 gk0 = *(const f32x4*)(k_gamma + dc * 8), gk1 = *(const f32x4*)(k_gamma + dc * 8 + 4);
  for (int base = threadIdx.x / LPR; base < n_items; base += U * RPB) {     // uniform over a lane group
    u32x4 x[U];
    unsigned short* bp[U];
    int which[U], hs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int it = base + u * RPB;
      if (it < n_items) {
        which[u] = it < H ? 0 : it < n_rope ? 1 : 2;      // 0 = q, 1 = k, 2 = v
        hs[u] = it - (which[u] == 0 ? 0 : which[u] == 1 ? H : n_rope);
        bp[u] = row + (which[u] == 0 ? 0 : which[u] == 1 ? k_off : v_off) + hs[u] * D;
        x[u] = *(const u32x4*)(bp[u] + dc * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int it = base + u * RPB;
      if (it >= n_items) continue;
      if (which[u] == 2) {
        *(u32x4*)(vc + (cache_row + (int64_t)hs[u] * max_len) * D + dc * 8) = x[u];
        continue;
      }
      float f[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f[2 * j] = __uint_as_float(x[u][j] << 16);
        f[2 * j + 1] = __uint_as_float(x[u][j] & 0xffff0000u);
      }
      float ss = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) ss = __fmaf_rn(f[j], f[j], ss);
#pragma unroll
      for (int o = 1; o < LPR; o <<= 1) ss = __fadd_rn(ss, __shfl_xor(ss, o, 64));
      const float r = rsqrtf(__fadd_rn(__fmul_rn(ss, 1.0f / D), eps));
      const f32x4 g0 = which[u] ? gk0 : gq0, g1 = which[u] ? gk1 : gq1;
      u32x4 n, pn;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float ga = j < 2 ? g0[2 * j] : g1[2 * j - 4], gb = j < 2 ? g0[2 * j + 1] : g1[2 * j - 3];
        n[j] = pack_bf16x2(__fmul_rn(__fmul_rn(f[2 * j], r), ga), __fmul_rn(__fmul_rn(f[2 * j + 1], r), gb));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) pn[j] = __shfl_xor(n[j], LPR / 2, 64);
      u32x4 olo, ohi;
      rope_rot8(upper ? pn : n, upper ? n : pn, c0, c1, s0, s1, olo, ohi);
      const u32x4 o = upper ? ohi : olo;
      *(u32x4*)(bp[u] + dc * 8) = o;
      if (which[u] == 1 && kc) *(u32x4*)(kc + (cache_row + (int64_t)hs[u] * max_len) * D + dc * 8) = o;
    }
  }
}

}  // namespace

extern "C" int icl_qknorm_rope_kv_bf16(void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const float* q_gamma,
                                       const float* k_gamma, float eps, const float* cosT, const float* sinT, const int32_t* pos,
                                       const int32_t* seq_ids, void* kcache, void* vcache, int32_t M, int32_t n_heads,
                                       int32_t n_kv_heads, int32_t head_dim, int32_t max_len, void* stream) {
  ICL_CHECK_ARG(qkv && cosT && sinT && pos, "icl_qknorm_rope_kv_bf16: NULL pointer");
  ICL_CHECK_ARG(q_gamma && k_gamma, "icl_qknorm_rope_kv_bf16: q_gamma and k_gamma must both be set");
  ICL_CHECK_ARG(M > 0 && n_heads > 0, "icl_qknorm_rope_kv_bf16: M and n_heads must be > 0");
  ICL_CHECK_ARG(head_dim == 64 || head_dim == 128, "icl_qknorm_rope_kv_bf16: head_dim=%d (only 64 and 128)", head_dim);
  ICL_CHECK_ARG(eps > 0.f, "icl_qknorm_rope_kv_bf16: eps must be > 0 (an all-zero head row would give NaN)");
  ICL_CHECK_ARG(n_kv_heads > 0 && n_heads % n_kv_heads == 0,
                "icl_qknorm_rope_kv_bf16: n_heads=%d is not a multiple of n_kv_heads=%d", n_heads, n_kv_heads);
  ICL_CHECK_ARG(ld % 8 == 0 && k_off % 8 == 0 && v_off % 8 == 0 && ((uintptr_t)qkv & 15) == 0,
                "icl_qknorm_rope_kv_bf16: qkv must be 16-byte aligned with ld/k_off/v_off multiples of 8");
  ICL_CHECK_ARG(k_off >= (int64_t)n_heads * head_dim && v_off >= k_off + (int64_t)n_kv_heads * head_dim &&
                    ld >= v_off + (int64_t)n_kv_heads * head_dim,
                "icl_qknorm_rope_kv_bf16: the q | k | v column blocks must be disjoint inside a row");
  ICL_CHECK_ARG(((uintptr_t)cosT & 15) == 0 && ((uintptr_t)sinT & 15) == 0 && ((uintptr_t)q_gamma & 15) == 0 &&
                    ((uintptr_t)k_gamma & 15) == 0, "icl_qknorm_rope_kv_bf16: cos / sin / gamma misaligned");
  ICL_CHECK_ARG((kcache == nullptr) == (vcache == nullptr),
                "icl_qknorm_rope_kv_bf16: kcache and vcache must both be set or both NULL");
  if (kcache) {
    ICL_CHECK_ARG(seq_ids && max_len > 0, "icl_qknorm_rope_kv_bf16: cache append needs seq_ids and max_len");
    ICL_CHECK_ARG(((uintptr_t)kcache & 15) == 0 && ((uintptr_t)vcache & 15) == 0, "icl_qknorm_rope_kv_bf16: cache misaligned");
  }
#define ICL_QKNORM(DD)                                                                                                          \
  hipLaunchKernelGGL((qknorm_rope_kv_kernel<DD>), dim3(M), dim3(256), 0, (hipStream_t)stream, (unsigned short*)qkv, ld, k_off, \
                     v_off, q_gamma, k_gamma, eps, cosT, sinT, pos, seq_ids, (unsigned short*)kcache, (unsigned short*)vcache, \
                     n_heads, n_kv_heads, max_len)
  if (head_dim == 64) ICL_QKNORM(64); else ICL_QKNORM(128);
#undef ICL_QKNORM
  ICL_CHECK_LAUNCH("icl_qknorm_rope_kv_bf16");
  return ICL_OK;
}

// rope_kv.hip — RoPE + KV-cache append outside a GEMM epilogue (gfx950): the rotation of q / k in a fused QKV row and the write
// of k / v into the cache, with the per-head q / k RMSNorm of a QK-norm decoder (Qwen3) in front of it or the e4m3fn rounding
// of an FP8 KV cache behind it.  Contracts and numerics: include/icl_hip.h (icl_rope_kv_bf16, icl_rope_kv_gqa_bf16,
// icl_qknorm_rope_kv_bf16 and, under "FP8 KV cache", icl_rope_kv_fp8 and icl_kv_append_fp8).  Two kernels, one block per qkv row:
//
// rope_kv_kernel: a thread holds the 8 low and the 8 high elements of a rotation, for any head_dim % 16 == 0 (the two plain bf16
// entry points).
//
// rope_kv_rows_kernel<D, NORM, F8, ROPE>: a head row (q, k or v of one head) is held by LPR = D / 8 adjacent lanes, lane dc its
// elements 8 dc .. 8 dc + 7 (one 16-B load), so a block works on 256 / LPR head rows at a time and U = 2 of them per thread per
// pass: 32 head rows a pass at head_dim 128, 64 at head_dim 64.  All of a pass's loads are issued before the first use; cos / sin
// (ROPE) and the two gamma chunks (NORM) depend on the lane alone and are loaded once per block.  Per head row, in this order:
//
// NORM (q and k rows).  Sum of squares, the documented order: a lane adds the squares of its eight elements in element order,
// s = 0, s += x[j]^2 for j = 0 .. 7 (a bf16 square is exact in f32, so the fused and the separate form of that step are the same
// number); the LPR partial sums are then folded by an xor butterfly over lane distances 1, 2, .. LPR / 2, so every lane of the
// group holds the same ss.  r = rsqrtf(ss * (1 / D) + eps);  n[i] = bf16_rne((x[i] * r) * gamma[i]).
// ROPE (q and k rows).  The rotation needs element i and i + D / 2: lane dc takes its partner's chunk from lane dc ^ (LPR / 2) by
// shuffle, both run rope_rot8 on the same eight pairs and each keeps the half it owns — the function and the bf16 rounding points
// of rope_kv_kernel (on a buffer holding n, with NORM).  In place: q always; k in the bf16 forms (an FP8 form leaves the k block
// of qkv as it was, and without ROPE it never writes qkv: the prefill QKV GEMM has rotated k in its epilogue).
// F8 (k and v rows).  kv_fp8_quant8: the row maximum by an xor butterfly over the same LPR lanes, the scale 2^e, eight e4m3fn codes
// per lane; 8 B of codes per lane and the scale from lane 0 go to the planes, unless pos[m] is outside [0, max_len): then the row
// stores nothing.  Otherwise the 16-B chunk goes to the bf16 cache as it is (no position guard, as in rope_kv_kernel).  No LDS.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), no scratch and no LDS in any of them:
//     <D, NORM, F8, ROPE>          VGPRs  SGPRs  waves per SIMD      (the same figures at D = 64 and D = 128)
//     <D, 1, 0, 1>  QK-norm          68     46        7
//     <D, 0, 1, 1>  FP8 rotate       60     52        8
//     <D, 0, 1, 0>  FP8 append       43     44        8
// rope_kv_kernel: 88 VGPRs, 56 SGPRs, 5 waves per SIMD.
#include <type_traits>
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// RoPE (HF rotate_half pairing) in place on q,k of a fused QKV row + KV-cache append.
// One block per row; work items of 8 elements (16 B).
__global__ __launch_bounds__(256) void rope_kv_kernel(unsigned short* qkv, int64_t ld, int64_t k_off,
                                                       int64_t v_off, const float* cosT,
                                                       const float* sinT, const int* pos,
                                                       const int* seq_ids, unsigned short* kc,
                                                       unsigned short* vc, int H, int Hkv, int D, int max_len) {
  // H query heads; Hkv heads in the k / v blocks and in the cache (grouped-query attention: Hkv < H, icl_rope_kv_gqa_bf16)
  const int64_t m = blockIdx.x;
  const int p = pos[m];
  const int half = D >> 1;
  const int per_head = half >> 3;          // 8-element items per (tensor, head)
  const int q_items = H * per_head;
  const int rope_items = q_items + Hkv * per_head; // q and k
  unsigned short* row = qkv + m * ld;
  const int64_t cache_row = kc ? ((int64_t)seq_ids[m] * Hkv) * max_len + p : 0;
  // Two rope items and two V items per thread per pass, ALL loads issued before the first use: with one small block per
  // row the kernel is latency-bound on bytes in flight per thread (2.8 TB/s with the loads interleaved with their uses).
  constexpr int U = 2;
  const int v_items = vc ? Hkv * (D >> 3) : 0;
  for (int base = threadIdx.x; base < rope_items || base < v_items; base += U * blockDim.x) {
    u32x4 lo[U], hi[U], vv[U];
    f32x4 c0[U], c1[U], s0[U], s1[U];
    unsigned short* rb[U];
    int i0s[U], hs[U], whichs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int it = base + u * blockDim.x;
      if (it < rope_items) {
        const int which = it >= q_items;                // 0 = q, 1 = k
        const int rem = it - which * q_items;
        const int h = rem / per_head, i0 = (rem - h * per_head) * 8;
        unsigned short* bp = row + (which ? k_off : 0) + h * D;
        rb[u] = bp; i0s[u] = i0; hs[u] = h; whichs[u] = which;
        lo[u] = *(const u32x4*)(bp + i0);
        hi[u] = *(const u32x4*)(bp + i0 + half);
        c0[u] = *(const f32x4*)(cosT + (int64_t)p * half + i0);
        c1[u] = *(const f32x4*)(cosT + (int64_t)p * half + i0 + 4);
        s0[u] = *(const f32x4*)(sinT + (int64_t)p * half + i0);
        s1[u] = *(const f32x4*)(sinT + (int64_t)p * half + i0 + 4);
      }
      if (it < v_items) {
        const int h = it / (D >> 3), i0 = (it - h * (D >> 3)) * 8;
        vv[u] = *(const u32x4*)(row + v_off + h * D + i0);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int it = base + u * blockDim.x;
      if (it < rope_items) {
        u32x4 olo, ohi;
        rope_rot8(lo[u], hi[u], c0[u], c1[u], s0[u], s1[u], olo, ohi);
        *(u32x4*)(rb[u] + i0s[u]) = olo;
        *(u32x4*)(rb[u] + i0s[u] + half) = ohi;
        if (whichs[u] == 1 && kc) {
          unsigned short* dst = kc + (cache_row + (int64_t)hs[u] * max_len) * D;
          *(u32x4*)(dst + i0s[u]) = olo;
          *(u32x4*)(dst + i0s[u] + half) = ohi;
        }
      }
      if (it < v_items) {
        const int h = it / (D >> 3), i0 = (it - h * (D >> 3)) * 8;
        *(u32x4*)(vc + (cache_row + (int64_t)h * max_len) * D + i0) = vv[u];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The head-row kernel (file header).  H query heads, Hkv heads in the k / v blocks and the cache.  kc / vc: the bf16 K and V rows
// (both NULL: no append), or with F8 the two e4m3fn byte planes; their f32 scale planes ks, vs are the trailing arguments of the
// FP8 forms alone, so the QK-norm form has the argument list of the kernel it came from, type for type (a cache argument that
// differed from it, as a struct or as unused trailing pointers, measured 0.3 - 0.5 us slower per launch at one row:
// profiles/r12_rope_kv_unify.txt).
template <int D, bool NORM, bool F8, bool ROPE, class... Scales>
__global__ __launch_bounds__(256) void rope_kv_rows_kernel(unsigned short* qkv, int64_t ld, int64_t k_off, int64_t v_off,
                                                           const float* q_gamma, const float* k_gamma, float eps,
                                                           const float* cosT, const float* sinT, const int* pos,
                                                           const int* seq_ids, std::conditional_t<F8, unsigned char, unsigned short>* kc,
                                                           decltype(kc) vc, int H, int Hkv, int max_len, Scales... scales) {
  constexpr int LPR = D / 8, HALF = D / 2, RPB = 256 / LPR, U = 2;
  const int64_t m = blockIdx.x;
  const int p = pos[m];
  const int dc = threadIdx.x % LPR;
  const bool upper = dc >= LPR / 2;                       // this lane owns elements of the second half of the head row
  const int i0 = (dc % (LPR / 2)) * 8;                    // the eight (i, i + HALF) pairs this lane rotates
  unsigned short* row = qkv + m * ld;
  const int64_t cache_row = kc ? ((int64_t)seq_ids[m] * Hkv) * max_len + p : 0;
  const int n_q = ROPE ? H : 0;                           // head rows: q heads (not without ROPE: nothing is done to q),
  const int n_rope = n_q + Hkv;                           // k heads, then (with a cache) v heads
  const int n_items = n_rope + (vc ? Hkv : 0);
  f32x4 c0 = {}, c1 = {}, s0 = {}, s1 = {}, gq0 = {}, gq1 = {}, gk0 = {}, gk1 = {};
  if constexpr (ROPE) {
    const float* cp = cosT + (int64_t)p * HALF + i0;
    const float* sp = sinT + (int64_t)p * HALF + i0;
    c0 = *(const f32x4*)cp, c1 = *(const f32x4*)(cp + 4), s0 = *(const f32x4*)sp, s1 = *(const f32x4*)(sp + 4);
  }
  if constexpr (NORM) {
    gq0 = *(const f32x4*)(q_gamma + dc * 8), gq1 = *(const f32x4*)(q_gamma + dc * 8 + 4);
    gk0 = *(const f32x4*)(k_gamma + dc * 8), gk1 = *(const f32x4*)(k_gamma + dc * 8 + 4);
  }
  for (int base = threadIdx.x / LPR; base < n_items; base += U * RPB) {     // uniform over a lane group
    u32x4 x[U];
    unsigned short* bp[U];
    int which[U], hs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int it = base + u * RPB;
      if (it < n_items) {
        which[u] = it < n_q ? 0 : it < n_rope ? 1 : 2;    // 0 = q, 1 = k, 2 = v
        hs[u] = it - (which[u] == 0 ? 0 : which[u] == 1 ? n_q : n_rope);
        bp[u] = row + (which[u] == 0 ? 0 : which[u] == 1 ? k_off : v_off) + hs[u] * D;
        x[u] = *(const u32x4*)(bp[u] + dc * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int it = base + u * RPB;
      if (it >= n_items) continue;
      u32x4 o = x[u];
      if (which[u] != 2) {
        if constexpr (NORM) {
          float f[8];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            f[2 * j] = __uint_as_float(o[j] << 16);
            f[2 * j + 1] = __uint_as_float(o[j] & 0xffff0000u);
          }
          float ss = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) ss = __fmaf_rn(f[j], f[j], ss);
#pragma unroll
          for (int d = 1; d < LPR; d <<= 1) ss = __fadd_rn(ss, __shfl_xor(ss, d, 64));
          const float r = rsqrtf(__fadd_rn(__fmul_rn(ss, 1.0f / D), eps));
          const f32x4 g0 = which[u] ? gk0 : gq0, g1 = which[u] ? gk1 : gq1;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float ga = j < 2 ? g0[2 * j] : g1[2 * j - 4], gb = j < 2 ? g0[2 * j + 1] : g1[2 * j - 3];
            o[j] = pack_bf16x2(__fmul_rn(__fmul_rn(f[2 * j], r), ga), __fmul_rn(__fmul_rn(f[2 * j + 1], r), gb));
          }
        }
        if constexpr (ROPE) {
          u32x4 po, olo, ohi;
#pragma unroll
          for (int j = 0; j < 4; ++j) po[j] = __shfl_xor(o[j], LPR / 2, 64);
          rope_rot8(upper ? po : o, upper ? o : po, c0, c1, s0, s1, olo, ohi);
          o = upper ? ohi : olo;
        }
        if (which[u] == 0 || !F8) *(u32x4*)(bp[u] + dc * 8) = o;
        if (which[u] == 0) continue;
      }
      const int64_t r = cache_row + (int64_t)hs[u] * max_len;               // the cache row of this k / v head row
      if constexpr (F8) {
        u32x2 q;
        float sc;
        kv_fp8_quant8<LPR>(o, q, sc);
        if (p >= 0 && p < max_len) {
          float* const planes[] = {scales...};                              // ks, vs
          *(u32x2*)((which[u] == 1 ? kc : vc) + r * D + dc * 8) = q;
          if (dc == 0) planes[which[u] - 1][r] = sc;
        }
      } else if (kc) {
        *(u32x4*)((which[u] == 1 ? kc : vc) + r * D + dc * 8) = o;
      }
    }
  }
}

// One call's arguments: what every form has, in the order of the entry points' lists, then what only some have.
struct RopeKvArgs {
  void* qkv;
  int64_t ld, k_off, v_off;
  const float *cosT, *sinT;
  const int32_t *pos, *seq_ids;
  void *kc, *vc;                                    // bf16 caches, or the e4m3fn byte planes
  int32_t M, H, Hkv, D, max_len;
  void* stream;
  const float *q_gamma = nullptr, *k_gamma = nullptr;   // FORM_NORM
  float eps = 0.f;
  float *ks = nullptr, *vs = nullptr;               // FORM_F8: the scale planes
};
// What an entry point's form has.  FORM_BLOCKS: the q | k | v column blocks are checked to be disjoint (every entry point but
// icl_rope_kv_bf16); FORM_NORM: gamma + eps; FORM_F8: FP8 planes, which must be set (otherwise bf16 caches, which may both be NULL);
// FORM_ROPE: cos / sin.  FORM_NORM or FORM_F8 is the head-row kernel, head_dim 64 or 128; neither is rope_kv_kernel, any
// head_dim % 16 == 0.
enum : unsigned { FORM_BLOCKS = 1, FORM_NORM = 2, FORM_F8 = 4, FORM_ROPE = 8 };

// The checks of every form in one order.  icl_rope_kv_gqa_bf16 used to test its head counts and column blocks first: a call that
// is wrong in several ways may now name another of them first (n_heads <= 0: "M and n_heads must be > 0").
int rope_kv_check(const char* who, unsigned form, const RopeKvArgs& a) {
  const bool norm = form & FORM_NORM, f8 = form & FORM_F8;
  const auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  if (f8) ICL_CHECK_ARG(a.qkv && a.pos && a.seq_ids && a.kc && a.vc && a.ks && a.vs, "%s: NULL pointer", who);
  else ICL_CHECK_ARG(a.qkv && a.cosT && a.sinT && a.pos, "%s: NULL pointer", who);
  if (norm) ICL_CHECK_ARG(a.q_gamma && a.k_gamma, "%s: q_gamma and k_gamma must both be set", who);
  if (f8) ICL_CHECK_ARG(a.M > 0 && a.H > 0 && a.max_len > 0, "%s: M, n_heads and max_len must be > 0", who);
  else ICL_CHECK_ARG(a.M > 0 && a.H > 0, "%s: M and n_heads must be > 0", who);
  if (norm || f8) ICL_CHECK_ARG(a.D == 64 || a.D == 128, "%s: head_dim=%d (only 64 and 128)", who, a.D);
  else ICL_CHECK_ARG(a.D % 16 == 0 && a.D >= 16, "%s: head_dim=%d must be a multiple of 16", who, a.D);
  if (norm) ICL_CHECK_ARG(a.eps > 0.f, "%s: eps must be > 0 (an all-zero head row would give NaN)", who);
  ICL_CHECK_ARG(a.Hkv > 0 && a.H % a.Hkv == 0, "%s: n_heads=%d is not a multiple of n_kv_heads=%d", who, a.H, a.Hkv);
  ICL_CHECK_ARG(a.ld % 8 == 0 && a.k_off % 8 == 0 && a.v_off % 8 == 0 && al16(a.qkv),
                "%s: qkv must be 16-byte aligned with ld/k_off/v_off multiples of 8", who);
  if (form & FORM_BLOCKS)
    ICL_CHECK_ARG(a.k_off >= (int64_t)a.H * a.D && a.v_off >= a.k_off + (int64_t)a.Hkv * a.D && a.ld >= a.v_off + (int64_t)a.Hkv * a.D,
                  "%s: %sq | k | v column blocks must be disjoint inside a row", who, f8 ? "" : "the ");
  if (f8) {
    ICL_CHECK_ARG(al16(a.kc) && al16(a.vc) && ((uintptr_t)a.ks & 3) == 0 && ((uintptr_t)a.vs & 3) == 0, "%s: cache misaligned", who);
    if (form & FORM_ROPE) ICL_CHECK_ARG(a.cosT && a.sinT && al16(a.cosT) && al16(a.sinT), "%s: cos/sin NULL or misaligned", who);
    return ICL_OK;
  }
  if (norm) ICL_CHECK_ARG(al16(a.cosT) && al16(a.sinT) && al16(a.q_gamma) && al16(a.k_gamma), "%s: cos / sin / gamma misaligned", who);
  else ICL_CHECK_ARG(al16(a.cosT) && al16(a.sinT), "%s: cos/sin misaligned", who);
  ICL_CHECK_ARG((a.kc == nullptr) == (a.vc == nullptr), "%s: kcache and vcache must both be set or both NULL", who);
  if (a.kc) {
    ICL_CHECK_ARG(a.seq_ids && a.max_len > 0, "%s: cache append needs seq_ids and max_len", who);
    ICL_CHECK_ARG(al16(a.kc) && al16(a.vc), "%s: cache misaligned", who);
  }
  return ICL_OK;
}

// The one launcher of the head-row kernel.  Only what has an entry point is instantiated: norm + rope, f8 + rope and f8 alone, at
// head_dim 64 and 128.
template <int D>
void rope_kv_rows_launch(unsigned form, const RopeKvArgs& a) {
  const dim3 grid(a.M), block(256);
  hipStream_t st = (hipStream_t)a.stream;
  unsigned char *kq = (unsigned char*)a.kc, *vq = (unsigned char*)a.vc;
#define ROWS_HEAD (unsigned short*)a.qkv, a.ld, a.k_off, a.v_off, a.q_gamma, a.k_gamma, a.eps, a.cosT, a.sinT, a.pos, a.seq_ids
#define ROWS_TAIL a.H, a.Hkv, a.max_len
  if (form & FORM_NORM)
    hipLaunchKernelGGL((rope_kv_rows_kernel<D, true, false, true>), grid, block, 0, st, ROWS_HEAD, (unsigned short*)a.kc,
                       (unsigned short*)a.vc, ROWS_TAIL);
  else if (form & FORM_ROPE)
    hipLaunchKernelGGL((rope_kv_rows_kernel<D, false, true, true, float*, float*>), grid, block, 0, st, ROWS_HEAD, kq, vq, ROWS_TAIL,
                       a.ks, a.vs);
  else
    hipLaunchKernelGGL((rope_kv_rows_kernel<D, false, true, false, float*, float*>), grid, block, 0, st, ROWS_HEAD, kq, vq, ROWS_TAIL,
                       a.ks, a.vs);
#undef ROWS_HEAD
#undef ROWS_TAIL
}

int rope_kv_run(const char* who, unsigned form, const RopeKvArgs& a) {
  if (const int rc = rope_kv_check(who, form, a)) return rc;
  if (form & (FORM_NORM | FORM_F8))
    a.D == 64 ? rope_kv_rows_launch<64>(form, a) : rope_kv_rows_launch<128>(form, a);
  else
    hipLaunchKernelGGL(rope_kv_kernel, dim3(a.M), dim3(256), 0, (hipStream_t)a.stream, (unsigned short*)a.qkv, a.ld, a.k_off, a.v_off,
                       a.cosT, a.sinT, a.pos, a.seq_ids, (unsigned short*)a.kc, (unsigned short*)a.vc, a.H, a.Hkv, a.D, a.max_len);
  ICL_CHECK_LAUNCH(who);
  return ICL_OK;
}

}  // namespace

extern "C" int icl_rope_kv_bf16(void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const float* cosT, const float* sinT,
                                const int32_t* pos, const int32_t* seq_ids, void* kcache, void* vcache, int32_t M, int32_t n_heads,
                                int32_t head_dim, int32_t max_len, void* stream) {
  return rope_kv_run("icl_rope_kv_bf16", FORM_ROPE,
                     {qkv, ld, k_off, v_off, cosT, sinT, pos, seq_ids, kcache, vcache, M, n_heads, n_heads, head_dim, max_len, stream});
}

extern "C" int icl_rope_kv_gqa_bf16(void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const float* cosT, const float* sinT,
                                    const int32_t* pos, const int32_t* seq_ids, void* kcache, void* vcache, int32_t M,
                                    int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, int32_t max_len, void* stream) {
  return rope_kv_run("icl_rope_kv_gqa_bf16", FORM_BLOCKS | FORM_ROPE,
                     {qkv, ld, k_off, v_off, cosT, sinT, pos, seq_ids, kcache, vcache, M, n_heads, n_kv_heads, head_dim, max_len, stream});
}

extern "C" int icl_qknorm_rope_kv_bf16(void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const float* q_gamma,
                                       const float* k_gamma, float eps, const float* cosT, const float* sinT, const int32_t* pos,
                                       const int32_t* seq_ids, void* kcache, void* vcache, int32_t M, int32_t n_heads,
                                       int32_t n_kv_heads, int32_t head_dim, int32_t max_len, void* stream) {
  RopeKvArgs a = {qkv, ld, k_off, v_off, cosT, sinT, pos, seq_ids, kcache, vcache, M, n_heads, n_kv_heads, head_dim, max_len, stream};
  a.q_gamma = q_gamma, a.k_gamma = k_gamma, a.eps = eps;
  return rope_kv_run("icl_qknorm_rope_kv_bf16", FORM_BLOCKS | FORM_NORM | FORM_ROPE, a);
}

extern "C" int icl_rope_kv_fp8(void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const float* cosT, const float* sinT,
                               const int32_t* pos, const int32_t* seq_ids, void* kq, void* vq, float* kscale, float* vscale,
                               int32_t M, int32_t n_heads, int32_t head_dim, int32_t max_len, void* stream) {
  RopeKvArgs a = {qkv, ld, k_off, v_off, cosT, sinT, pos, seq_ids, kq, vq, M, n_heads, n_heads, head_dim, max_len, stream};
  a.ks = kscale, a.vs = vscale;
  return rope_kv_run("icl_rope_kv_fp8", FORM_BLOCKS | FORM_F8 | FORM_ROPE, a);
}

extern "C" int icl_kv_append_fp8(const void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const int32_t* pos, const int32_t* seq_ids,
                                 void* kq, void* vq, float* kscale, float* vscale, int32_t M, int32_t n_heads, int32_t head_dim,
                                 int32_t max_len, void* stream) {
  RopeKvArgs a = {(void*)qkv, ld, k_off, v_off, nullptr, nullptr, pos, seq_ids, kq, vq, M, n_heads, n_heads, head_dim, max_len, stream};
  a.ks = kscale, a.vs = vscale;
  return rope_kv_run("icl_kv_append_fp8", FORM_BLOCKS | FORM_F8, a);
}

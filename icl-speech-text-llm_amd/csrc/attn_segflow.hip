// attn_segflow.hip — the segment-to-segment attention flow readout: for EVERY prompt row i of a sequence, its causal softmax
// weights over the K cache, summed by (segment of the query row, segment of the key).  Flash-shaped; V is never read.
//
//   flow[b][h][a][c] = sum_{i < len, seg[i] = a} sum_{j <= i, seg[j] = c} p(i, j),   p(i, .) = softmax_{j <= i}(scale q_i . k_j)
//
// Structure (the score stage is attn.hip's attn_fwd_kernel, copied; the P.V product is replaced):
//   * one workgroup of 4 waves per (sequence, query head) walks the sequence's 128-query blocks in order; a wave owns 32 query rows
//     of a block, K tiles of 64 keys go through LDS (two buffers, one barrier per tile: tile t+1 is fetched to registers above
//     tile t's arithmetic and stored below it).  Query head h reads K head h / G; G is a kernel argument, not an instantiation.
//   * swapped QK^T: S^T = K . Q^T on v_mfma_f32_32x32x16_bf16 — the query sits on the LANE, its scores in the lane's accumulator
//     registers, the online (m, l) per lane (row maxima in plain C++: see attn.hip on why not inline asm).  The causal mask and
//     the j < len mask sit in the score stage.
//   * F^T = E^T . P^T with the accumulator as operand: E is the one-hot [key x 32 segments] matrix of the tile.  The converted
//     S^T registers 8s..8s+7 are the B operand of k-step s; the A operand is built in registers: lane (r = lane & 31, half) holds
//     seg[key] == r ? 1.0 : 0.0 for the eight keys 16s + 8(j>>2) + 4 half + (j&3), the k order those registers have.
//     P is NOT rounded once to bf16: p = hi + lo with hi = bf16_rne(p), lo = bf16_rne(p - hi) (p - hi is exact in f32, so
//     |p - hi - lo| <= 2^-18 p), two MFMAs per k-step.  F^T is rescaled by the lane's alpha per tile and divided by its l at the end.
//   * query-segment sums: a wave transposes its finished 32-query F^T block through a private LDS region and adds query i's
//     32-vector into row seg[i] of its own [32][32] f32 accumulator, in position order; the four accumulators are merged in wave
//     order at the end.  No atomics, no cross-workgroup reduction; every element of flow is written.
// Determinism: one instantiation per head_dim whatever the grid and G; which keys a lane folds and every summation order depend
// on the sequence's own length and ids only — a sequence's flow has the same bits alone and in any batch.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   attn_segflow_kernel<64>    VGPRs 142, AGPRs 32, SGPRs 54, LDS 51840 B, scratch 0, 2 waves / SIMD
//   attn_segflow_kernel<128>   VGPRs 173, AGPRs 32, SGPRs 54, LDS 68224 B, scratch 0, 2 waves / SIMD
#include "common.h"

namespace {

constexpr float SF_NEG_BIG = -1.0e30f;
constexpr float SF_LOG2E = 1.4426950408889634f;
constexpr int SF_MAX_SEG = 32;

// Row maxima use plain fmaxf; they must NOT be inline asm (attn.hip: hipcc's hazard recogniser does not look inside asm statements,
// and a vector instruction that reads an MFMA result needs software wait states on gfx950).
__device__ __forceinline__ float sf_max32(const f32x16& a, const f32x16& b) {
  float m = __builtin_fmaxf(a[0], a[1]);
#pragma unroll
  for (int r = 2; r < 16; ++r) m = __builtin_fmaxf(m, a[r]);
#pragma unroll
  for (int r = 0; r < 16; ++r) m = __builtin_fmaxf(m, b[r]);
  return m;
}

// max of a value with its partner in the other half of the wave (lane ^ 32), in every lane: one v_permlane32_swap
__device__ __forceinline__ float sf_max_xhalf(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  const unsigned lo = r[0], hi = r[1];
  return __builtin_fmaxf(__builtin_bit_cast(float, lo), __builtin_bit_cast(float, hi));
}

// four segment bytes -> four bf16 of the one-hot operand (1.0 = 0x3f80 where the byte is this lane's segment), two per dword
__device__ __forceinline__ u32x2 sf_onehot4(unsigned w, unsigned mine) {
  const unsigned e0 = (w & 255u) == mine ? 0x3f80u : 0u, e1 = ((w >> 8) & 255u) == mine ? 0x3f800000u : 0u;
  const unsigned e2 = ((w >> 16) & 255u) == mine ? 0x3f80u : 0u, e3 = (w >> 24) == mine ? 0x3f800000u : 0u;
  return u32x2{e0 | e1, e2 | e3};
}

// blockIdx.x = query head, blockIdx.y = sequence
template <int D>
__global__ __launch_bounds__(256) void attn_segflow_kernel(const unsigned short* Q, int64_t ldq, const int* cu, const unsigned short* Kc,
                                                            const unsigned char* seg, int64_t ld_seg, int n_seg, float* flow,
                                                            int n_heads, int n_kv_heads, int kv_group, int max_len,
                                                            float scale_log2e) {
  constexpr int KS = D / 16;                 // QK^T k-steps
  constexpr int CPR = D / 8;                 // 16-B chunks per K row
  constexpr int NCH = 64 * CPR / 256;        // chunks per thread per tile
  constexpr int PITCH = D * 2 + 16;          // bytes per K row in LDS (padded: rows 32 apart in one read do not share banks)
  constexpr int TP = 33;                     // floats per row of a wave's transposition region
  __shared__ __attribute__((aligned(16))) char k_lds[2][64 * PITCH];
  __shared__ __attribute__((aligned(16))) unsigned char seg_lds[2][64];
  __shared__ float tr_lds[4][32 * TP];       // per wave: F[query][segment] of its finished block
  __shared__ float acc_lds[4][32 * 32];      // per wave: [segment of the query][segment of the key]

  const int h = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ql = lane & 31, hh = lane >> 5;
  const int row0 = cu[b];
  const int len = min(cu[b + 1] - row0, max_len);
  float* out = flow + ((int64_t)b * n_heads + h) * (int64_t)(n_seg * n_seg);
#pragma unroll
  for (int i = 0; i < 16; ++i) acc_lds[wave][lane + 64 * i] = 0.f;    // a wave zeroes its own accumulator: in order before its adds
  if (len > 0) {     // cu ascending with at least one row per sequence is the contract; nothing is read otherwise
  const unsigned short* kbase = Kc + ((int64_t)b * n_kv_heads + h / kv_group) * (int64_t)max_len * D;
  const unsigned char* segb = seg + (int64_t)b * ld_seg;
  float* trw = tr_lds[wave];
  float* accw = acc_lds[wave];

  // this thread's share of a K tile: chunk c = tid + 256 i -> row c / CPR, 16-B slot c % CPR; and (tid < 64) one segment byte
  u32x4 kreg[NCH];
  unsigned sreg = 255u;
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = tid + 256 * i;
      const int64_t grow = min(k0 + c / CPR, len - 1);      // rows past the end are masked; the read stays inside the sequence
      kreg[i] = *(const u32x4*)(kbase + grow * D + (c % CPR) * 8);
    }
    if (tid < 64) sreg = k0 + tid < len ? (unsigned)segb[k0 + tid] : 255u;
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = tid + 256 * i;
      *(u32x4*)(k_lds[buf] + (c / CPR) * PITCH + (c % CPR) * 16) = kreg[i];
    }
    if (tid < 64) seg_lds[buf][tid] = (unsigned char)sreg;
  };

  for (int qb = 0; qb < len; qb += 128) {
    const int n_tiles = (min(len, qb + 128) + 63) >> 6;
    const int qw = qb + wave * 32;           // first query of this wave's block
    const int qpos = qw + ql;                // this lane's query
    const bool wave_has_q = qw < len;        // wave-uniform
    bf16x8 qf[KS];                           // Q fragments (B operand of S^T = K Q^T): lane (q, hh) holds Q[q][16ks + 8hh .. +7]
    {
      const unsigned short* qp = Q + (int64_t)(row0 + min(qpos, len - 1)) * ldq + (int64_t)h * D + hh * 8;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const bf16x8*)(qp + ks * 16);
    }
    const unsigned qseg = qpos < len ? (unsigned)segb[qpos] : 255u;     // the segment of this lane's query row
    f32x16 f_acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) f_acc[r] = 0.f;
    float m_run = SF_NEG_BIG, l_run = 0.f;

    gload(0);
    lstore(0);
    __syncthreads();
    for (int t = 0; t < n_tiles; ++t) {
      const int cur = t & 1, k0 = t * 64;
      if (t + 1 < n_tiles) gload(k0 + 64);
      // wave-uniform: does this wave's block hold a query and see a key of this tile?
      if (wave_has_q && k0 <= qw + 31) {
        // ---- S^T = K Q^T ----------------------------------------------------------------------------------------------
        f32x16 s_acc[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) s_acc[kb][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
          for (int kb = 0; kb < 2; ++kb) {
            const bf16x8 kf = *(const bf16x8*)(k_lds[cur] + (kb * 32 + ql) * PITCH + (2 * ks + hh) * 16);
            s_acc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s_acc[kb], 0, 0, 0);
          }
        // ---- scores -> base-2 logits, mask, online softmax ------------------------------------------------------------------
        const bool need_mask = (k0 + 64 > len) || (k0 + 63 > qw);       // wave-uniform
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = k0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            float v = s_acc[kb][r] * scale_log2e;
            if (need_mask) v = (key < len && key <= qpos) ? v : SF_NEG_BIG;
            s_acc[kb][r] = v;
          }
        const float tmax = sf_max_xhalf(sf_max32(s_acc[0], s_acc[1]));
        const float m_new = __builtin_fmaxf(m_run, tmax);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        bf16x8 pf[2][2], pl[2][2];           // the two-term bf16 split of the unnormalised weights
        float psum = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float e = __builtin_amdgcn_exp2f(s_acc[kb][r] - m_new);
            e = (s_acc[kb][r] <= SF_NEG_BIG * 0.5f) ? 0.f : e;
            psum += e;
            pf[kb][r >> 3][r & 7] = (__bf16)e;
            pl[kb][r >> 3][r & 7] = (__bf16)(e - (float)pf[kb][r >> 3][r & 7]);
          }
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int r = 0; r < 16; ++r) f_acc[r] *= alpha;
        // ---- F^T += E^T P^T -------------------------------------------------------------------------------------------------
        // A operand of k-step (kb, s): lane (r = ql, hh), element j <-> key kb*32 + 16s + 8(j>>2) + 4hh + (j&3): two runs of four
        // consecutive segment bytes, at kb*32 + 16s + 4hh and 8 further
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const unsigned char* sp = seg_lds[cur] + kb * 32 + 16 * s + 4 * hh;
            const u32x2 a0 = sf_onehot4(*(const unsigned*)sp, (unsigned)ql), a1 = sf_onehot4(*(const unsigned*)(sp + 8), (unsigned)ql);
            const bf16x8 ef = __builtin_bit_cast(bf16x8, u32x4{a0[0], a0[1], a1[0], a1[1]});
            f_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ef, pf[kb][s], f_acc, 0, 0, 0);
            f_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ef, pl[kb][s], f_acc, 0, 0, 0);
          }
      }
      if (t + 1 < n_tiles) lstore(cur ^ 1);      // that buffer held tile t-1: last read before the previous barrier
      __syncthreads();
    }
    // ---- this wave's block: F[q][c] = F^T[c][q] / l through the wave's LDS region, then into row seg[q], in position order -----
    if (wave_has_q) {
      const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
      const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) trw[ql * TP + (r & 3) + 8 * (r >> 2) + 4 * hh] = f_acc[r] * inv;
      __builtin_amdgcn_wave_barrier();           // same wave, in-order LDS queue
#pragma unroll 4
      for (int q = 0; q < 32; ++q) {
        const unsigned a = __shfl(qseg, q, 64);  // wave-uniform; 255 past the end of the sequence
        if (a < (unsigned)n_seg && hh == 0) accw[a * 32 + ql] += trw[q * TP + ql];
      }
      __builtin_amdgcn_wave_barrier();           // the next block's writes to the region come after these reads
    }
  }
  }
  __syncthreads();
  // ---- merge the four waves' accumulators in wave order; every element of flow[b][h] is written ----------------------------------
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = tid + 256 * i, a = e >> 5, c = e & 31;      // 1024 elements [a][c], four per thread
    if (a < n_seg && c < n_seg) out[a * n_seg + c] = ((acc_lds[0][e] + acc_lds[1][e]) + acc_lds[2][e]) + acc_lds[3][e];
  }
}

}  // namespace

extern "C" int icl_attn_segflow_bf16(const void* Q, int64_t ldq, const int32_t* cu, const void* Kc, const uint8_t* seg, int64_t ld_seg,
                                     int32_t n_seg, float* flow, int32_t n_seqs, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim,
                                     int32_t max_len, int32_t max_seqlen, float scale, void* stream) {
  ICL_CHECK_ARG(Q != nullptr, "icl_attn_segflow_bf16: Q is NULL");
  ICL_CHECK_ARG(cu != nullptr, "icl_attn_segflow_bf16: cu is NULL");
  ICL_CHECK_ARG(Kc != nullptr, "icl_attn_segflow_bf16: Kc is NULL");
  ICL_CHECK_ARG(seg != nullptr, "icl_attn_segflow_bf16: seg is NULL");
  ICL_CHECK_ARG(flow != nullptr, "icl_attn_segflow_bf16: flow is NULL");
  ICL_CHECK_ARG(n_seg >= 1 && n_seg <= SF_MAX_SEG, "icl_attn_segflow_bf16: n_seg=%d (1..%d)", n_seg, SF_MAX_SEG);
  ICL_CHECK_ARG(head_dim == 64 || head_dim == 128, "icl_attn_segflow_bf16: head_dim=%d (only 64 and 128)", head_dim);
  ICL_CHECK_ARG(n_seqs > 0 && n_seqs <= 65535, "icl_attn_segflow_bf16: n_seqs=%d (1..65535)", n_seqs);
  ICL_CHECK_ARG(n_heads > 0 && max_len > 0, "icl_attn_segflow_bf16: bad sizes (n_heads=%d, max_len=%d)", n_heads, max_len);
  if (n_kv_heads == 0) n_kv_heads = n_heads;
  ICL_CHECK_ARG(n_kv_heads > 0 && n_heads % n_kv_heads == 0,
                "icl_attn_segflow_bf16: n_heads=%d is not a multiple of n_kv_heads=%d", n_heads, n_kv_heads);
  const int group = n_heads / n_kv_heads;
  ICL_CHECK_ARG(group <= 8, "icl_attn_segflow_bf16: n_kv_heads=%d gives %d query heads per K/V head (at most 8)", n_kv_heads, group);
  ICL_CHECK_ARG(group == 1 || head_dim == 128,
                "icl_attn_segflow_bf16: n_kv_heads=%d with head_dim=%d (grouped-query attention: only 128)", n_kv_heads, head_dim);
  ICL_CHECK_ARG(max_seqlen >= 1 && max_seqlen <= max_len, "icl_attn_segflow_bf16: max_seqlen=%d (1..max_len=%d)", max_seqlen, max_len);
  ICL_CHECK_ARG(ld_seg >= max_len, "icl_attn_segflow_bf16: ld_seg=%lld < max_len=%d", (long long)ld_seg, max_len);
  ICL_CHECK_ARG(ldq % 8 == 0 && ldq >= (int64_t)n_heads * head_dim,
                "icl_attn_segflow_bf16: ldq=%lld must be a multiple of 8 and hold n_heads * head_dim columns", (long long)ldq);
  ICL_CHECK_ARG(((uintptr_t)Q & 15) == 0, "icl_attn_segflow_bf16: Q is not 16-byte aligned");
  ICL_CHECK_ARG(((uintptr_t)Kc & 15) == 0, "icl_attn_segflow_bf16: Kc is not 16-byte aligned");
  ICL_CHECK_ARG(((uintptr_t)flow & 3) == 0, "icl_attn_segflow_bf16: flow is not 4-byte aligned");
  ICL_CHECK_ARG(__builtin_isfinite(scale), "icl_attn_segflow_bf16: scale is not finite");
  const dim3 grid(n_heads, n_seqs);
  if (head_dim == 64)
    hipLaunchKernelGGL(attn_segflow_kernel<64>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned short*)Q, ldq, cu,
                       (const unsigned short*)Kc, seg, ld_seg, n_seg, flow, n_heads, n_kv_heads, group, max_len, scale * SF_LOG2E);
  else
    hipLaunchKernelGGL(attn_segflow_kernel<128>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned short*)Q, ldq, cu,
                       (const unsigned short*)Kc, seg, ld_seg, n_seg, flow, n_heads, n_kv_heads, group, max_len, scale * SF_LOG2E);
  ICL_CHECK_LAUNCH("icl_attn_segflow_bf16");
  return ICL_OK;
}

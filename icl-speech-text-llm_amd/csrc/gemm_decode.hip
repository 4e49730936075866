// gemm_decode.hip — the decode-step GEMM kernels for gfx950: weights streamed once, HBM -> VGPR in MFMA operand order.
//   * gemm_skinny_kernel (tiles 4 / 6) and gemm_skinny_fp8w_kernel (icl_gemm_fp8w): M <= 64; two entry points that share their
//     K range and activation set-up (inline functions) but each carry a copy of the combine + epilogue tail;
//   * gemm_m128_kernel (tile 5): M <= 256 on the decode-packed copy, 64- / 128- / 256-row blocks;
//   * the packers that make the decode-packed and the fp8 decode-packed copies (icl_pack_decode_weights, icl_pack_fp8_weights).
// Argument checks, tile selection and the GEMM entry points are in gemm.hip; it reaches these kernels through launch_skinny and
// launch_decode_tile (gemm_common.h).
#include "gemm_common.h"
#include <vector>

using namespace iclg;

namespace {

// =================================================================================================================
// Skinny GEMM for decode (M <= 64): the weight matrix is streamed ONCE, straight from HBM into VGPRs (no LDS round
// trip, no barriers in the stream: guide §5 table row "GEMV / M <= 16 decode"), 16 B per lane, several KiB in flight per
// wave.  Block = 8 waves = one 16*NT-column slab of the output; the waves split K eight ways and combine their 16x16
// f32 partial tiles through LDS (in-block split-K: deterministic, no workspace, no second launch).  The activations
// (M x K, <= 0.7 MB) are re-read by every block from L2.  MB = 16-row blocks of M, NT = 16-column tiles per block
// (2 for the SwiGLU epilogue so a gate block and its up block meet in one lane).
// =================================================================================================================
// ---- set-up shared by the two skinny entry points (bf16 and fp8 weights): written once.  Their combine + epilogue tails are still
// ---- two textual copies that must stay in step: as a shared inline function hipcc allocates registers differently and the
// ---- decode-packed <1,1,8> kernel measured 4-5 % slower on down_proj (profiles/r05_skinny_shared_ab.txt) ----------------------
// the per-wave range [s0, s1) of 32-wide k-steps: wave w of 8
__device__ __forceinline__ void skinny_krange(int K, int wave, int& s0, int& s1) {
  const int steps = K >> 5;
  s0 = (int)(((int64_t)wave * steps) >> 3);
  s1 = (int)(((int64_t)(wave + 1) * steps) >> 3);
}

// activation pointers (row clamped to M - 1; this lane's 8 k of a k-step) and zeroed accumulators
template <int MB, int NT>
__device__ __forceinline__ void skinny_setup(const __bf16* A, int M, int64_t lda, int fr, int fq, const __bf16* (&ap)[MB], f32x4 (&acc)[NT][MB]) {
#pragma unroll
  for (int b = 0; b < MB; ++b) ap[b] = A + (int64_t)min(b * 16 + fr, M - 1) * lda + fq * 8;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int b = 0; b < MB; ++b) acc[t][b] = f32x4{0.f, 0.f, 0.f, 0.f};
}

template <int MB, int NT, int U, bool PACKED>   // PACKED: W is the decode-packed copy (tile 6): a wave-load is 1 KB contiguous
__global__ __launch_bounds__(512) void gemm_skinny_kernel(GemmParams p) {
  __shared__ float red[8][NT][MB][256];   // [wave][n-tile][m-block][lane*4 + r]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int n0 = blockIdx.x * (16 * NT);
  int s0, s1;
  skinny_krange(p.K, wave, s0, s1);

  const __bf16* wp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
    wp[t] = PACKED ? p.W + (int64_t)min((n0 >> 4) + t, ((p.N + 15) >> 4) - 1) * (p.K >> 5) * 512 + lane * 8
                   : p.W + (int64_t)min(n0 + t * 16 + fr, p.N - 1) * p.ldw + fq * 8;
  constexpr int WSTEP = PACKED ? 512 : 32;   // elements between consecutive 32-wide k-steps of one n-tile
  const __bf16* ap[MB];
  f32x4 acc[NT][MB];
  skinny_setup<MB, NT>(p.A, p.M, p.lda, fr, fq, ap, acc);

  int s = s0;
  for (; s + U <= s1; s += U) {
    bf16x8 wf[U][NT], af[U][MB];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int t = 0; t < NT; ++t) wf[u][t] = *(const bf16x8*)(wp[t] + (int64_t)(s + u) * WSTEP);
#pragma unroll
      for (int b = 0; b < MB; ++b) af[u][b] = *(const bf16x8*)(ap[b] + (int64_t)(s + u) * 32);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int b = 0; b < MB; ++b)
          acc[t][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u][t], af[u][b], acc[t][b], 0, 0, 0);
  }
  for (; s < s1; ++s) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const bf16x8 wf = *(const bf16x8*)(wp[t] + (int64_t)s * WSTEP);
#pragma unroll
      for (int b = 0; b < MB; ++b) {
        const bf16x8 af = *(const bf16x8*)(ap[b] + (int64_t)s * 32);
        acc[t][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af, acc[t][b], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int b = 0; b < MB; ++b) *(f32x4*)&red[wave][t][b][lane * 4] = acc[t][b];
  __syncthreads();
  // 8 waves share the NT*MB output fragments
  for (int f = wave; f < NT * MB; f += 8) {
    const int t = f / MB, b = f - t * MB;
    f32x4 v = *(const f32x4*)&red[0][t][b][lane * 4];
#pragma unroll
    for (int w = 1; w < 8; ++w) v = v + *(const f32x4*)&red[w][t][b][lane * 4];
    if (!(p.epi & ICL_EPI_SWIGLU)) epi_store4(p, 0, b * 16 + fr, n0 + t * 16 + fq * 4, v);
    else *(f32x4*)&red[0][t][b][lane * 4] = v;
  }
  if (p.epi & ICL_EPI_SWIGLU) {
    if constexpr (NT == 2) {
      __syncthreads();
      for (int b = wave; b < MB; b += 8) {
        const f32x4 g = *(const f32x4*)&red[0][0][b][lane * 4], u = *(const f32x4*)&red[0][1][b][lane * 4];
        epi_store_swiglu(p, 0, b * 16 + fr, n0, fq * 4, g, u);
      }
    }
  }
}

// ---- the fp8-weight form of the skinny kernel (FP8 weight mode: see the packer below): an entry point of its own because it
// ---- takes the row scales; set-up is skinny_krange / skinny_setup, the tail a copy of gemm_skinny_kernel's ---------------------
// 8 e4m3fn codes (two dwords, element k in byte k) -> bf16 fragment of q * sc (sc = 2^e_n of this lane's row: every step exact)
__device__ __forceinline__ bf16x8 fp8x8_scaled_bf16(unsigned lo, unsigned hi, float sc) {
  const f32x2 s = {sc, sc};
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(lo, false) * s, b = __builtin_amdgcn_cvt_pk_f32_fp8(lo, true) * s;
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false) * s, d = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true) * s;
  return bf16x8{(__bf16)a[0], (__bf16)a[1], (__bf16)b[0], (__bf16)b[1], (__bf16)c[0], (__bf16)c[1], (__bf16)d[0], (__bf16)d[1]};
}

// gemm_skinny_kernel<MB, NT, U, true> on the fp8 decode-packed copy: same block shape, same per-wave K split (k-steps s0 .. s1 - 1
// of 32), same MFMA order per accumulator (k-step ascending), same wave-0..7 combine and epilogues (a copy: keep the two in step).  A wave-load is 16 B per lane =
// two k-steps, so a wave walks the k-PAIRS that overlap its range and skips the half-pair outside it at either end (wave-uniform
// branches).  U k-pairs are loaded per batch; the batch past the end re-reads the wave's last pair (in bounds, never used).
template <int MB, int NT, int U>
__global__ __launch_bounds__(512) void gemm_skinny_fp8w_kernel(GemmParams p, const float* __restrict__ wscale) {
  __shared__ float red[8][NT][MB][256];   // [wave][n-tile][m-block][lane*4 + r]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int n0 = blockIdx.x * (16 * NT);
  int s0, s1;
  skinny_krange(p.K, wave, s0, s1);
  const int j0 = s0 >> 1, j1 = (s1 + 1) >> 1;

  const unsigned char* wp[NT];
  float sc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    wp[t] = (const unsigned char*)p.W + (int64_t)min((n0 >> 4) + t, ((p.N + 15) >> 4) - 1) * (p.K >> 6) * 1024 + lane * 16;
    sc[t] = wscale[min(n0 + t * 16 + fr, p.N - 1)];
  }
  const __bf16* ap[MB];
  f32x4 acc[NT][MB];
  skinny_setup<MB, NT>(p.A, p.M, p.lda, fr, fq, ap, acc);

  for (int j = j0; j < j1; j += U) {
    u32x4 wq[U][NT];
    bf16x8 af[U][2][MB];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int jj = min(j + u, j1 - 1);
#pragma unroll
      for (int t = 0; t < NT; ++t) wq[u][t] = *(const u32x4*)(wp[t] + (int64_t)jj * 1024);
#pragma unroll
      for (int b = 0; b < MB; ++b) {
        af[u][0][b] = *(const bf16x8*)(ap[b] + (int64_t)jj * 64);
        af[u][1][b] = *(const bf16x8*)(ap[b] + (int64_t)jj * 64 + 32);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (j + u >= j1) break;
      const int s = 2 * (j + u);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (h == 0 ? s < s0 : s + 1 >= s1) continue;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const bf16x8 wf = fp8x8_scaled_bf16(wq[u][t][2 * h], wq[u][t][2 * h + 1], sc[t]);
#pragma unroll
          for (int b = 0; b < MB; ++b) acc[t][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af[u][h][b], acc[t][b], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int b = 0; b < MB; ++b) *(f32x4*)&red[wave][t][b][lane * 4] = acc[t][b];
  __syncthreads();
  // 8 waves share the NT*MB output fragments
  for (int f = wave; f < NT * MB; f += 8) {
    const int t = f / MB, b = f - t * MB;
    f32x4 v = *(const f32x4*)&red[0][t][b][lane * 4];
#pragma unroll
    for (int w = 1; w < 8; ++w) v = v + *(const f32x4*)&red[w][t][b][lane * 4];
    if (!(p.epi & ICL_EPI_SWIGLU)) epi_store4(p, 0, b * 16 + fr, n0 + t * 16 + fq * 4, v);
    else *(f32x4*)&red[0][t][b][lane * 4] = v;
  }
  if (p.epi & ICL_EPI_SWIGLU) {
    if constexpr (NT == 2) {
      __syncthreads();
      for (int b = wave; b < MB; b += 8) {
        const f32x4 g = *(const f32x4*)&red[0][0][b][lane * 4], u = *(const f32x4*)&red[0][1][b][lane * 4];
        epi_store_swiglu(p, 0, b * 16 + fr, n0, fq * 4, g, u);
      }
    }
  }
}

// U per cell: k-steps (fp8: k-pairs) of weight and activation fragments a wave holds in flight, [row blocks 1 | 2 | 4][NT - 1][SkinnyW]
constexpr int SKINNY_U[3][2][3] = {
    {{8, 8, 8}, {4, 4, 4}},
    {{4, 4, 4}, {2, 2, 2}},
    {{2, 2, 2}, {2, 2, 1}},   // fp8 <4,2>: register pressure — a k-pair is two k-steps of activations; U = 1 already takes 104 VGPRs
};

template <int MBI, int NT>   // MBI: log2 of the row blocks (1 | 2 | 4)
int launch_skinny_cell(const GemmParams& p, SkinnyW form, const float* wscale, hipStream_t stream) {
  constexpr int MB = 1 << MBI;
  const dim3 grid((p.N + 16 * NT - 1) / (16 * NT)), block(512);
  if (form == SKINNY_W_FP8)
    hipLaunchKernelGGL((gemm_skinny_fp8w_kernel<MB, NT, SKINNY_U[MBI][NT - 1][SKINNY_W_FP8]>), grid, block, 0, stream, p, wscale);
  else if (form == SKINNY_W_PACKED)
    hipLaunchKernelGGL((gemm_skinny_kernel<MB, NT, SKINNY_U[MBI][NT - 1][SKINNY_W_PACKED], true>), grid, block, 0, stream, p);
  else
    hipLaunchKernelGGL((gemm_skinny_kernel<MB, NT, SKINNY_U[MBI][NT - 1][SKINNY_W_ROW], false>), grid, block, 0, stream, p);
  ICL_CHECK_LAUNCH(form == SKINNY_W_FP8 ? "icl_gemm_fp8w" : "icl_gemm_bf16(skinny)");
  return ICL_OK;
}

// =================================================================================================================
// Decode GEMM for 64 < M <= 128 (tile id 5).  At this size a decode GEMM sits on the ridge: 2*128 FLOP per weight
// byte, i.e. the 13.5 GB of Llama-7B weights cost about the same on the matrix pipe as on HBM, and what decides is how
// much a CU has to move per weight byte: through its vector-memory path (measured ceiling here ~55-68 GB/s per CU) and
// out of LDS (128 B/clk).  The 64x64 LDS tile moves 3 bytes per weight byte (W once, the activation slice twice as
// much again from L2) and reads 4 bytes of LDS; this kernel moves 2 and reads 4 — but of a tile twice as wide:
//   * one block = ALL (<= 128) rows x 128 columns.  Its 8 waves are 4 column groups (32 columns = two 16-wide n-tiles,
//     so a SwiGLU gate block and its up block meet in one lane) x 2 K-halves: wave (wc, wk) takes the 32-wide k-step
//     wk of every 64-wide K-tile.  Every weight byte is loaded by exactly one wave, and each wave reads only its half
//     of the staged activations (splitting the columns 8 ways instead would have every wave read all of them: LDS-bound
//     at 0.59 us per K-tile).  The two K-halves meet once, through LDS, after the loop (fixed order: even + odd);
//   * W goes HBM -> VGPR directly in MFMA operand order from the decode-packed copy (icl_pack_decode_weights): per
//     16-row n-tile a K-long stream of 1-KB pieces, one per 32-wide k-step, so a wave-load is 1 KB contiguous, lane l
//     at byte 16*l.  (Row-major W read in operand order is 16 rows x 64 B per wave-load = 64 separate L1 accesses; that
//     pattern capped the first version of this kernel and caps the skinny kernel.)  DEPTH K-tiles deep in registers;
//   * A (shared by all waves) is staged by LDS-DMA into a DEPTH+1 ring, one barrier per K-tile;
//   * loads past the end of the K range are clamped to its last tile, so the in-flight count (vmcnt) is the same in
//     every iteration and no tail code exists;
//   * split-K over grid.z with the same workspace slabs + reduce kernel as the other tiles; with split_k == 1 the bias
//     is folded into the accumulator init like everywhere else.
template <int DEPTH, int MT>   // DEPTH: K-tiles of W in registers (and of A in LDS, + 1 being read); MT: 16-row tiles (8 | 4)
__global__ __launch_bounds__(512) void gemm_m128_kernel(GemmParams p) {
  constexpr int NI = 2, BN = 4 * NI * 16, A_INSTR = MT / 4, A_STAGE = MT * 16 * 128, NSA = DEPTH + 1;
  constexpr int G = A_INSTR + NI;   // VMEM loads per K-tile per lane
  static_assert(MT == 16 || MT == 8 || MT == 4, "256-, 128- or 64-row blocks");
  static_assert(NSA * A_STAGE >= 4 * MT * NI * 1024, "the K-half exchange reuses the A ring");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wave & 3, wk = wave >> 2;
  const int n0 = blockIdx.x * BN, z = blockIdx.z;
  const int nk = p.K >> 6;
  int kt0 = 0, kt1 = nk;
  if (p.split_k > 1) {
    kt0 = (int)(((int64_t)z * nk) / p.split_k);
    kt1 = (int)(((int64_t)(z + 1) * nk) / p.split_k);
  }
  const int nt = kt1 - kt0;
  const int fr = lane & 15, fq = lane >> 4;

  const __bf16* ga[A_INSTR];
#pragma unroll
  for (int j = 0; j < A_INSTR; ++j) {
    const int row = (j * 8 + wave) * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ ((row >> 1) & 7);
    ga[j] = p.A + (int64_t)min(row, p.M - 1) * p.lda + (int64_t)kt0 * 64 + chunk * 8;
  }
  const int n_tiles16 = (p.N + 15) >> 4;
  const __bf16* gw[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j)
    gw[j] = p.W + ((int64_t)min((n0 >> 4) + wc * NI + j, n_tiles16 - 1) * (p.K >> 5) + (int64_t)kt0 * 2 + wk) * 512 + lane * 8;

  auto stage_a = [&](int t, int slot) {
    const int tc = min(t, nt - 1);
    char* base = smem + slot * A_STAGE + wave * 1024;
#pragma unroll
    for (int j = 0; j < A_INSTR; ++j)
      __builtin_amdgcn_global_load_lds((gptr_t)(ga[j] + (int64_t)tc * 64), (lptr_t)(base + j * 8 * 1024), 16, 0, 0);
  };
  bf16x8 wf[DEPTH][NI];
  auto load_w = [&](bf16x8 (&w)[NI], int t) {
    const int tc = min(t, nt - 1);
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      // raw loads: hipcc's waitcnt pass answers a loop-carried register load next to LDS-DMA with vmcnt(0) at the loop
      // header (the whole prefetch drained once per unrolled body); the counted wait in tile() covers these instead
      const __bf16* src = gw[j] + (int64_t)tc * 1024;
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(w[j]) : "v"(src) : "memory");
    }
  };
  const int a_off = fr * 128 + (((wk * 4 + fq) ^ (fr >> 1)) * 16);

  f32x4 acc[MT][NI];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // bias folded into the accumulator init exactly like the LDS tiles do ((bias + sum), residual last); K-half 0 carries it
  const bool fold_bias = p.split_k == 1 && vec_path_ok(p) && (p.epi & ICL_EPI_BIAS);
  if (fold_bias && wk == 0) {
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n = n0 + (wc * NI + j) * 16 + fq * 4;
      const f32x4 b4 = n < p.N ? *(const f32x4*)(p.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < MT; ++i) acc[i][j] = b4;
    }
  }

  int slot = 0;                              // ring slot of the K-tile being computed
  auto tile = [&](bf16x8 (&w)[NI], int t) {
    // the K-tile t operands are the oldest loads in flight; tiles t+1 .. t+DEPTH-1 (G loads each) may still be
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((DEPTH - 1) * G) : "memory");
    __builtin_amdgcn_s_barrier();            // A(t) of every wave has landed; every wave is done reading A(t-1)
    __builtin_amdgcn_sched_barrier(0);
    stage_a(t + DEPTH, slot == 0 ? NSA - 1 : slot - 1);   // into the ring slot of t-1
    const char* a_s = smem + slot * A_STAGE + a_off;
    slot = slot == NSA - 1 ? 0 : slot + 1;
    constexpr int MH = MT > 8 ? 8 : MT;      // activation fragments held at a time (256-row blocks take two passes: registers)
#pragma unroll
    for (int ih = 0; ih < MT / MH; ++ih) {
      bf16x8 af[MH];
#pragma unroll
      for (int i = 0; i < MH; ++i) af[i] = *(const bf16x8*)(a_s + (ih * MH + i) * 16 * 128);
#pragma unroll
      for (int i = 0; i < MH; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          acc[ih * MH + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[j], af[i], acc[ih * MH + i][j], 0, 0, 0);
      if (MT > MH) __builtin_amdgcn_sched_barrier(0);      // keep the second pass's fragment reads behind the first pass's MFMAs
    }
    __builtin_amdgcn_sched_barrier(0);
    load_w(w, t + DEPTH);                    // this register set is free again
    __builtin_amdgcn_sched_barrier(0);
  };

#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    stage_a(d, d);
    load_w(wf[d], d);
    __builtin_amdgcn_sched_barrier(0);
  }
  int t = 0;
  for (; t + DEPTH <= nt; t += DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) tile(wf[d], t + d);
  }
#pragma unroll
  for (int d = 0; d < DEPTH - 1; ++d)
    if (t + d < nt) tile(wf[d], t + d);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the clamped over-issue must not outlive the block's LDS
  // ... nor its registers: to the compiler a raw load's result is there at once, so a result nobody reads is a free
  // register while the load is still in flight.  Reading every set here keeps all of them allocated up to the wait.
#pragma unroll
  for (int s_ = 0; s_ < DEPTH; ++s_)
#pragma unroll
    for (int j = 0; j < NI; ++j) asm volatile("" ::"v"(wf[s_][j]));

  // ---- the two K-halves meet: odd half -> LDS (the A ring is dead), even half adds it on top and stores ---------------
  __syncthreads();
  char* xbase = smem + wc * (MT * NI * 1024) + lane * 16;
  if (wk == 1) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) *(f32x4*)(xbase + (i * NI + j) * 1024) = acc[i][j];
  }
  __syncthreads();
  if (wk == 1) return;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = acc[i][j] + *(const f32x4*)(xbase + (i * NI + j) * 1024);

  // ---- epilogue: acc[i][j][r] = C[m][n], m = i*16 + fr, n = n0 + (wc*NI + j)*16 + fq*4 + r ---------------------------
  GemmParams q = p;
  if (fold_bias) q.epi &= ~ICL_EPI_BIAS;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = i * 16 + fr;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int nt_ = n0 + (wc * NI + j) * 16;
      if (p.split_k > 1) {
        epi_store_partial(p, z, m, nt_ + fq * 4, acc[i][j]);
      } else if (p.epi & ICL_EPI_SWIGLU) {
        if ((j & 1) == 0) epi_store_swiglu(q, 0, m, nt_, fq * 4, acc[i][j], acc[i][(j + 1) % NI]);
      } else {
        epi_store4(q, 0, m, nt_ + fq * 4, acc[i][j]);
      }
    }
  }
}

template <int DEPTH, int MT>
int launch_m128(const GemmParams& p, hipStream_t stream) {
  constexpr int BN = 128, SMEM = (DEPTH + 1) * MT * 16 * 128;
  if (const int rc = allow_dynamic_lds<gemm_m128_kernel<DEPTH, MT>>(SMEM)) return rc;
  hipLaunchKernelGGL((gemm_m128_kernel<DEPTH, MT>), dim3((p.N + BN - 1) / BN, 1, p.split_k), dim3(512), SMEM, stream, p);
  ICL_CHECK_LAUNCH("icl_gemm_bf16(m128)");
  return ICL_OK;
}

// row-major W [N][ldw] -> decode-packed: piece (n-tile, k-step, lane = fq*16 + fr) holds W[16*nt + fr][32*ks + 8*fq .. +8]
__global__ __launch_bounds__(256) void pack_decode_w_kernel(const unsigned short* W, int64_t ldw, int N, int K, u32x4* out) {
  const int64_t pieces = (int64_t)((N + 15) >> 4) * (K >> 5) * 64;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < pieces; q += (int64_t)gridDim.x * 256) {
    const int l = (int)(q & 63);
    const int64_t blk = q >> 6;
    const int ks = (int)(blk % (K >> 5));
    const int64_t row = (blk / (K >> 5)) * 16 + (l & 15);
    out[q] = row < N ? *(const u32x4*)(W + row * ldw + ks * 32 + (l >> 4) * 8) : u32x4{0u, 0u, 0u, 0u};
  }
}

// =================================================================================================================
// FP8 weight mode (icl_pack_fp8_weights / icl_gemm_fp8w): the decoder's GEMM weights W are replaced by W' = q * 2^e_n, where
// e_n is the smallest integer with max_k |W[n][k]| <= 448 * 2^e_n (0 for an all-zero row) and q[n][k] = RNE_e4m3fn(W[n][k] / 2^e_n)
// (OCP e4m3fn; the division is exact and never saturates).  W' is exact in bf16 (4 significant bits, power-of-two scale).
// The decode kernel streams q (1 byte per weight) and rebuilds W' in registers: fp8 -> f32 (exact), * 2^e_n (exact: every lane
// of an MFMA weight fragment holds ONE output row, so the scale is per lane), -> bf16 (exact).  It then issues the MFMA sequence
// of the bf16 skinny kernel on those fragments, so its output is the bits tile 6 produces on the decode-packed copy of W'.
// =================================================================================================================
// fp8_row_exponent / f32_to_e4m3fn: common.h (shared with the FP8 KV cache)
// q * 2^e as bf16 bits (exact whenever the result is a bf16 normal)
__device__ __forceinline__ unsigned short e4m3fn_scaled_to_bf16(unsigned c, int e) {
  const int E = (c >> 3) & 15, M = c & 7;
  const float v = ldexpf((float)(E ? 8 + M : M), (E ? E - 1 : 0) - 9 + e);
  return f32_to_bf16_bits((c & 0x80u) ? -v : v);
}

// One block per 16-row n-tile.  Phase 1: row maxima (and a finiteness check) -> e_n, scales[n] = 2^e_n (NaN marks a row with a
// non-finite value; the host rejects the matrix).  Phase 2: the fp8 decode-packed pieces — piece (n-tile, k-pair j, lane = fq*16 + fr)
// is 16 B: q[16*nt + fr][64j + 8fq .. +8] then q[16*nt + fr][64j + 32 + 8fq .. +8] (two 32-wide k-steps; a wave-load is 1 KB
// contiguous, as in pack_decode_w_kernel) — and W' over the row-major matrix Wd (may be W itself: each thread rewrites only what
// it has read, after the block's maxima are known).
__global__ __launch_bounds__(256) void pack_fp8_w_kernel(const unsigned short* W, int64_t ldw, int N, int K, u32x4* q, float* scales,
                                                         unsigned short* Wd, int64_t ldd) {
  __shared__ int e_s[16];
  __shared__ int bad_s[16];
  const int nt = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int r = wave; r < 16; r += 4) {
    const int64_t row = (int64_t)nt * 16 + r;
    float m = 0.f, bad = 0.f;
    if (row < N) {
      for (int k = lane * 8; k < K; k += 512) {
        const u32x4 v = *(const u32x4*)(W + row * ldw + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float x0 = fabsf(__uint_as_float(v[j] << 16)), x1 = fabsf(__uint_as_float(v[j] & 0xffff0000u));
          if (!(x0 <= 3.4028235e38f) || !(x1 <= 3.4028235e38f)) bad = 1.f;
          m = fmaxf(m, fmaxf(x0, x1));
        }
      }
    }
    m = wave_reduce_max(m);
    bad = wave_reduce_max(bad);
    if (lane == 0) {
      const int e = fp8_row_exponent(m);
      e_s[r] = e;
      bad_s[r] = bad != 0.f;
      if (row < N) scales[row] = bad != 0.f ? __uint_as_float(0x7fc00000u) : ldexpf(1.f, e);
    }
  }
  __syncthreads();
  const int kp = K >> 6;
  for (int pi = tid; pi < kp * 64; pi += 256) {
    const int l = pi & 63, j = pi >> 6, fr = l & 15, fq = l >> 4;
    const int64_t row = (int64_t)nt * 16 + fr;
    u32x4 out = {0u, 0u, 0u, 0u};
    if (row < N && !bad_s[fr]) {
      const int e = e_s[fr];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int64_t k = (int64_t)j * 64 + h * 32 + fq * 8;
        const u32x4 v = *(const u32x4*)(W + row * ldw + k);
        u32x4 wd;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const unsigned c0 = f32_to_e4m3fn(ldexpf(__uint_as_float(v[i] << 16), -e));
          const unsigned c1 = f32_to_e4m3fn(ldexpf(__uint_as_float(v[i] & 0xffff0000u), -e));
          out[h * 2 + (i >> 1)] |= (c0 | (c1 << 8)) << ((i & 1) * 16);
          wd[i] = (unsigned)e4m3fn_scaled_to_bf16(c0, e) | ((unsigned)e4m3fn_scaled_to_bf16(c1, e) << 16);
        }
        *(u32x4*)(Wd + row * ldd + k) = wd;
      }
    }
    q[((int64_t)nt * kp + j) * 64 + l] = out;
  }
}

}  // namespace

// the skinny kernel's instantiation by (row blocks of 16, SwiGLU or not, weight form); the caller has checked M <= 64, batch == 1
int iclg::launch_skinny(const GemmParams& p, SkinnyW form, const float* wscale, hipStream_t stream) {
  const int mb = (p.M + 15) / 16;
  if (p.epi & ICL_EPI_SWIGLU)
    return mb <= 1 ? launch_skinny_cell<0, 2>(p, form, wscale, stream) : mb == 2 ? launch_skinny_cell<1, 2>(p, form, wscale, stream)
                                                                                 : launch_skinny_cell<2, 2>(p, form, wscale, stream);
  return mb <= 1 ? launch_skinny_cell<0, 1>(p, form, wscale, stream) : mb == 2 ? launch_skinny_cell<1, 1>(p, form, wscale, stream)
                                                                               : launch_skinny_cell<2, 1>(p, form, wscale, stream);
}

// tile 5 (M <= 256, checked by the caller): 64-row blocks stage half the A bytes of 128-row blocks; 256-row blocks (two micro-batches
// decoded together): a weight byte then serves twice the rows.  Depth 3 / 4 / 6 measured alike: the CU's vector-memory path is the
// limit, not latency.
int iclg::launch_decode_tile(const GemmParams& p, hipStream_t stream) {
  return p.M <= 64 ? launch_m128<3, 4>(p, stream) : p.M <= 128 ? launch_m128<3, 8>(p, stream) : launch_m128<3, 16>(p, stream);
}

extern "C" int icl_pack_decode_weights(const void* W, int64_t ldw, int32_t N, int32_t K, void* out, void* stream) {
  ICL_CHECK_ARG(W && out && N > 0 && K > 0, "icl_pack_decode_weights: bad arguments");
  ICL_CHECK_ARG(K % 64 == 0 && ldw % 8 == 0 && ldw >= K, "icl_pack_decode_weights: K=%d must be a multiple of 64, ldw=%lld a multiple of 8", K, (long long)ldw);
  ICL_CHECK_ARG(((uintptr_t)W & 15) == 0 && ((uintptr_t)out & 15) == 0, "icl_pack_decode_weights: misaligned pointer");
  const int64_t pieces = (int64_t)((N + 15) >> 4) * (K >> 5) * 64;
  const int blocks = (int)std::min<int64_t>((pieces + 255) / 256, 65535);
  hipLaunchKernelGGL(pack_decode_w_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)W, ldw, N, K, (u32x4*)out);
  ICL_CHECK_LAUNCH("icl_pack_decode_weights");
  return ICL_OK;
}

extern "C" int icl_pack_fp8_weights(const void* W, int64_t ldw, int32_t N, int32_t K, void* q, float* scales, void* w_deq,
                                    int64_t ld_deq, void* stream) {
  ICL_CHECK_ARG(W && q && scales && w_deq && N > 0 && K > 0, "icl_pack_fp8_weights: bad arguments");
  ICL_CHECK_ARG(K % 64 == 0 && ldw % 8 == 0 && ldw >= K && ld_deq % 8 == 0 && ld_deq >= K,
                "icl_pack_fp8_weights: K=%d must be a multiple of 64, ldw=%lld / ld_deq=%lld multiples of 8 and >= K", K, (long long)ldw,
                (long long)ld_deq);
  ICL_CHECK_ARG((((uintptr_t)W | (uintptr_t)q | (uintptr_t)w_deq) & 15) == 0, "icl_pack_fp8_weights: misaligned pointer");
  ICL_CHECK_ARG(w_deq == W ? ld_deq == ldw : true, "icl_pack_fp8_weights: in place needs ld_deq == ldw");
  const int tiles = (N + 15) >> 4;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pack_fp8_w_kernel, dim3(tiles), dim3(256), 0, s, (const unsigned short*)W, ldw, N, K, (u32x4*)q, scales,
                     (unsigned short*)w_deq, ld_deq);
  ICL_CHECK_LAUNCH("icl_pack_fp8_weights");
  // a load-time call: it waits for its scales to report a non-finite weight (a NaN scale marks the row) as ICL_EINVAL
  std::vector<float> sc_host(N);
  hipError_t e = hipMemcpyAsync(sc_host.data(), scales, sizeof(float) * (size_t)N, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    icl_set_error("icl_pack_fp8_weights: %s", hipGetErrorString(e));
    return ICL_ELAUNCH;
  }
  for (int n = 0; n < N; ++n)
    ICL_CHECK_ARG(sc_host[n] == sc_host[n], "icl_pack_fp8_weights: row %d holds a non-finite value", n);
  return ICL_OK;
}

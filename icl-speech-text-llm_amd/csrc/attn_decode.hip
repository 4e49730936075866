// attn_decode.hip — single-token decode attention over the KV cache (HBM-bound KV stream): ONE kernel,
// attn_decode_kernel<D, UNR, FUSE, F8, EPL, NG, MASK, R>, behind every icl_attn_decode_* entry point and icl_attn_cut_rows_bf16.
// Cache layout [n_seqs][n_heads][max_len][D] bf16: the keys of one (sequence, head) are one
// contiguous stream, read with 16-B loads straight to VGPRs (no LDS round trip: guide §5 table row
// "GEMV / M <= 16 decode").  D/8 lanes cover one key row, so a wave-instruction fetches 64/(D/8)
// consecutive keys (1 KiB).  Every lane keeps an online-softmax stream (m, l, o[8]) for its
// (key slot, d-chunk); the 4*64/(D/8) streams of a block are merged once through LDS.
#include "common.h"

namespace {

constexpr float NEG_BIG = -1.0e30f;
constexpr float LOG2E = 1.4426950408889634f;

// D = head_dim (64 or 128).
// UNR = key rounds (4 * KPW keys each) whose K and V loads are issued before the first of them is consumed.  A stream's keys and
// their order do not depend on it: few workgroups (a small decode batch: one block per (sequence, head), nothing else on the CU to
// hide a 2-3 us round trip per loop iteration) take the deep unroll, a full chip 4.  (The instruction selection, and so FMA
// contraction, can differ between unrolls; instantiations compared bit for bit below use the same UNR.)
// FUSE (icl_attn_decode_rope_bf16): the step's RoPE + cache append run HERE instead of in a launch of their own (rope_kv_kernel:
// ~5 us per layer at any decode batch, one of the nine launches of a one-sequence decode layer).  Q holds the projection's raw
// q | k | v row of sequence b; every lane rotates the q chunk it needs (and the new key's chunk) with rope_rot8 — the function and
// the bf16 rounding points of rope_kv_kernel, so the result is bit-identical to the two launches — the first LPR lanes append the
// rotated key and the value to the cache at position pos[b], and in the key loop position pos[b] is served from registers, never
// from the cache line that is being written.
// EPL = elements of a key row per lane (LPR = D / EPL lanes per row).  The bf16 kernel takes 8 (one 16-B load).
// F8 (icl_attn_decode_fp8 / icl_attn_decode_rope_fp8): the cache holds e4m3fn bytes and one f32 scale 2^e per row (include/icl_hip.h,
// "FP8 KV cache").  A lane takes EPL = 16 elements — one 16-B load, so 8 lanes cover a 128-B row and a wave-instruction still
// reads 1 KiB — plus the row's scale, and rebuilds x' = q * 2^e as the bf16 words a bf16 cache holding x' would hold (exact) before
// the arithmetic (kv_words): fed f32 directly, the compiler contracts the dot products into FMAs differently than for bf16 words.
// So the output is bit-identical to the bf16 instantiation with EPL = 16 (icl_attn_decode_bf16_epl16, a reference entry point) on
// a bf16 cache of x'; against the production EPL = 8 kernel only the order of the d-chunk partial sums of each score differs.
// FUSE rounds the appended key and value to x' in registers (kv_fp8_quant: the row maximum is a shuffle over the row's LPR lanes)
// and serves the rounded row.
// NG (icl_attn_decode_gqa_bf16) = query heads per K/V head; 1 = multi-head attention.  One workgroup per (sequence, K/V head): a
// lane uses the K chunk and V chunk it loaded for all NG heads, so a cache row is read once for NG heads, a decode step streams
// 1 / NG of the bytes NG = 1 reads from the per-group expanded cache, and the output is NG = 1's on that cache up to the compiler's
// FMA contraction.  The state (q chunk, m, l, o[8]) is 18 VGPRs per head, so UNR shrinks as NG grows.  The K / V
// conversions (kv_words) stay inside the per-head loop, next to their uses: the identity for bf16, and hoisted out of it they cost
// the fp8 instantiations 43-85 VGPRs (196 -> 261 at <128, 8, false, true, 16>: a whole key group's converted rows live at once).
// MASK (icl_attn_decode_masked_bf16, attention knockout): a row LIST instead of all sequences and a per-key, per-head segment
// mask; bf16, no RoPE-fused and no fp8 form.  ONE UNR per (head_dim, group size), whatever the grid: the few / many switch of
// the unmasked multi-head launches changes bits (measured: a row alone at UNR 16 against the same row among 1056 workgroups at
// UNR 4), and a knockout result must not depend on the batch a row travels in.  Multi-head takes 8 — between the two: 116 VGPRs
// and 4 waves per SIMD, against 201 / 2 at UNR 16 and 102 / 4 at UNR 4 — grouped the unmasked kernel's UNR (the mask costs UNR
// bytes in flight and NG wave-uniform words).  -Rpass-analysis=kernel-resource-usage for gfx950, VGPRs / SGPRs / waves per
// SIMD, masked (the unmasked instantiation of the same <D, UNR, NG>); no instantiation uses scratch or spills a VGPR:
//   <64, 8, .., 1>    115 / 43 / 4                      <128, 8, .., 1>   116 / 43 / 4
//   <128, 8, .., 2>   160 / 43 / 3  (151 / 32 / 3)      <128, 4, .., 3>   125 / 54 / 4  (121 / 36 / 4)
//   <128, 4, .., 4>   152 / 59 / 3  (160 / 32 / 3)      <128, 4, .., 5>   169 / 76 / 2  (165 / 42 / 3)
//   <128, 4, .., 6>   212 / 91 / 2  (206 / 42 / 2)      <128, 4, .., 7>   241 / 104 / 2 (239 / 46 / 2)
//   <128, 4, .., 8>   256 + 3 AGPRs / 101 / 1  (254 / 32 / 2): UNR 4 is the smallest there is, so G = 8 runs one wave per SIMD
// R (icl_attn_cut_rows_bf16, attention cuts between prompt segments) > 0: a form of MASK over TILES of R listed rows of one cache
// sequence — hundreds of interior prompt rows per sequence, not one — so that one pass over the sequence's K / V stream serves R
// rows as it serves NG heads: R * NG states per lane, each with its own key count and mask.  ONE instantiation per (head_dim, G)
// whatever the grid and the list, UNR 4 (the grouped table's from three states on): a slot's bits are the same alone in a tile,
// in any slot, next to any companions.  R = 4 at G = 1, 2 at G = 2, 1 from G = 3 on (cut_tile_rows).  The same remark for
// <D, 4, .., NG, MASK, R>, VGPRs / SGPRs / waves per SIMD; no instantiation uses scratch or spills:
//   <64, 4, .., 1, 4>   194 / 54 / 2     <128, 4, .., 1, 4>  172 / 54 / 2     <128, 4, .., 2, 2>  144 / 52 / 3
//   <128, 4, .., 3, 1>  126 / 47 / 4     <128, 4, .., 4, 1>  144 / 51 / 3     <128, 4, .., 5, 1>  162 / 55 / 3
//   <128, 4, .., 6, 1>  212 / 53 / 2     <128, 4, .., 7, 1>  230 / 57 / 2     <128, 4, .., 8, 1>  248 / 61 / 2
// (four slots of one head hold more than four heads of one row — 172 against 152 VGPRs — because each slot brings its own key
// count into the predicate; still two waves per SIMD and no scratch, so R = 4 stays.)
struct DecodeRope {
  const float* cosT;
  const float* sinT;
  const int* pos;
  const int* seq_ids;     // cache row of sequence b (NULL: b)
  void* kc;               // the caches, writable (Kc / Vc of the kernel are these)
  void* vc;
  float* ks;              // F8: the row scales of kc / vc (Ks / Vs of the kernel)
  float* vs;
  int64_t k_off, v_off;   // column offsets of k / v in the qkv row
};

// MASK: the list and the per-key mask of icl_attn_decode_masked_bf16, behind the (unused, zero) DecodeRope of a MASK = false launch
struct DecodeMask : DecodeRope {
  const unsigned char* seg;   // seg[row_seq[r] * ld_seg + key]: the segment of a key
  int64_t ld_seg;
  const unsigned* blocked;    // blocked[r * (query heads) + head]: bit g = segment g is not read
  const int* row_seq;         // list entry r: the cache sequence ...
  const int* row_q;           // ... and the row of Q / O
};
// R > 0: the tiles of icl_attn_cut_rows_bf16 behind the mask's seg / ld_seg / blocked / row_q (row_seq unused), one entry per
// tile or per slot t * R + r
struct DecodeCut : DecodeMask {
  const int* tile_seq;            // [n_tiles]: the cache sequence of a tile
  const int* row_len;             // [n_tiles * R]: the keys a slot's query may see
  const unsigned char* head_on;   // [query heads] or NULL (all): a head that is off is not written
};
template <bool MASK, int R> struct DecodeTail { typedef DecodeRope T; };
template <> struct DecodeTail<true, 0> { typedef DecodeMask T; };
template <int R> struct DecodeTail<true, R> { typedef DecodeCut T; };

template <int EPL> struct KvWords;                       // EPL bf16 of a lane: EPL / 2 dwords
template <> struct KvWords<8> { typedef u32x4 T; };
template <> struct KvWords<16> { typedef u32x8 T; };
template <bool F8, int EPL> struct KvRaw { typedef typename KvWords<EPL>::T T; };   // a lane's cache bytes: bf16 words ...
template <> struct KvRaw<true, 16> { typedef u32x4 T; };                              // ... or 16 e4m3fn codes

// a lane's EPL cache elements as bf16 words (F8: x' = q * sc, exact in bf16)
template <bool F8, int EPL>
__device__ __forceinline__ typename KvWords<EPL>::T kv_words(typename KvRaw<F8, EPL>::T r, float sc) {
  if constexpr (F8) {
    const unsigned qs[4] = {r[0], r[1], r[2], r[3]};
    float f[16];
    kv_fp8_deq<4>(qs, sc, f);
    typename KvWords<EPL>::T w;
#pragma unroll
    for (int t = 0; t < 8; ++t) w[t] = pack_bf16x2(f[2 * t], f[2 * t + 1]);
    return w;
  } else {
    return r;
  }
}

// blockIdx.x = h, a head of the CACHE (n_heads of them); its query heads are h * NG + g.
// MASK (icl_attn_decode_masked_bf16): blockIdx.y = r, an entry of a row LIST — cache sequence row_seq[r], row row_q[r] of Q / O —
// and key j of query head hq counts iff j < len and not (seg_j < 32 and bit seg_j of blocked[r][hq]): the predicate joins ok[i].
// One segment byte per key a lane group loads (UNR bytes in flight next to the UNR K / V rows); the NG masks of a K/V group are
// wave-uniform (SGPRs) and each head's own mask meets the shared K / V chunk inside the per-head loop.  A stream folds the keys
// the unmasked kernel gives it, in its groups of four: a masked key is a key past the end, s = NEG_BIG and p = 0.
// R > 0 (icl_attn_cut_rows_bf16, attention cuts): blockIdx.y = t, a TILE of R slots — listed rows of ONE cache sequence tile_seq[t],
// slot r being entry t * R + r of row_q / row_len / blocked (row_q < 0: an empty slot) — and the NG loop runs over the R * NG
// queries (slot r, head g of the group) that share the loaded K / V chunk.  The block walks keys 0 .. max row_len of its live
// slots - 1 once; key j counts for a state iff j < row_len[slot] and not blocked by the slot's mask, so the keys a slot meets past
// its own row_len are keys past the end (s = NEG_BIG, p = 0: m, l and o keep their bits; a group of four wholly past it is not
// entered).  Heads that are off and empty slots are not written; a K/V group whose heads are all off returns at once.
template <int D, int UNR, bool FUSE, bool F8, int EPL, int NG, bool MASK = false, int R = 0>
__global__ __launch_bounds__(256) void attn_decode_kernel(const unsigned short* Q, int64_t ldq, const void* Kc, const void* Vc,
                                                           const float* Ks, const float* Vs, unsigned short* O, int64_t ldo,
                                                           const int* lens, int n_heads, int max_len, float scale_log2e,
                                                           typename DecodeTail<MASK, R>::T rp) {
  typedef typename KvRaw<F8, EPL>::T Raw;
  typedef typename KvWords<EPL>::T Wd;
  static_assert(!F8 || EPL == 16, "the fp8 cache is read 16 elements per lane");
  static_assert(NG == 1 || (!FUSE && !F8 && D == 128 && EPL == 8), "grouped-query: the plain bf16 form at head_dim 128 only");
  static_assert(!MASK || (!FUSE && !F8 && EPL == 8), "masked: the plain bf16 forms only");
  static_assert(R == 0 || MASK, "row tiles: a form of the masked kernel");
  constexpr bool TILE = R > 0;
  constexpr int NQ = (TILE ? R : 1) * NG;   // online-softmax states of a lane: one per (slot, head of the group)
  constexpr int NW = EPL / 2;      // bf16 words per lane
  constexpr int EB = F8 ? 1 : 2;   // bytes per cache element
  constexpr int LPR = D / EPL;     // lanes per key row
  constexpr int KPW = 64 / LPR;    // keys per wave-instruction
  constexpr int NSTREAM = 4 * KPW;
  __shared__ float sm[NSTREAM][D + 2];  // per stream of ONE head: o[D], m, l
  const int h = blockIdx.x, b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dc = lane % LPR, sub = lane / LPR;
  int bs = b, bq = b;              // the cache sequence, and the row of Q / O
  unsigned blk[NQ] = {};
  int rq[NQ], qlen[NQ];            // TILE: the row of Q / O of a state's slot, and the keys its query may see (0: nothing to do)
  const unsigned char* segp = nullptr;
  int len;
  if constexpr (TILE) {
    bs = rp.tile_seq[b];
    unsigned on = 0;
#pragma unroll
    for (int g = 0; g < NG; ++g) on |= (rp.head_on == nullptr || rp.head_on[h * NG + g]) ? 1u << g : 0u;
    if (!on) return;
    len = 0;
#pragma unroll
    for (int x = 0; x < NQ; ++x) {
      const int e = b * R + x / NG;
      rq[x] = rp.row_q[e];
      const bool live = rq[x] >= 0 && ((on >> (x % NG)) & 1u);
      qlen[x] = live ? min(rp.row_len[e], max_len) : 0;
      if (!live) rq[x] = -1;
      blk[x] = rp.blocked[e];
      len = max(len, qlen[x]);
    }
    if (len <= 0) return;
    segp = rp.seg + (int64_t)bs * rp.ld_seg;
  } else if constexpr (MASK) {
    bs = rp.row_seq[b];
    bq = rp.row_q[b];
#pragma unroll
    for (int g = 0; g < NG; ++g) blk[g] = rp.blocked[((int64_t)b * n_heads + h) * NG + g];
    segp = rp.seg + (int64_t)bs * rp.ld_seg;
  }
  if constexpr (!TILE) len = min(lens[bs], max_len);
  const int crow = FUSE && rp.seq_ids ? rp.seq_ids[b] : bs;
  const int64_t base = ((int64_t)crow * n_heads + h) * (int64_t)max_len * D;
  const int64_t sbase = base / D;     // F8: the scale of row (crow, h, key) is Ks[sbase + key]
  const char* kp = (const char*)Kc + (base + dc * EPL) * EB;
  const char* vp = (const char*)Vc + (base + dc * EPL) * EB;

  Wd q_raw[NQ];
  Raw k_new = {}, v_new = {};
  float ks_new = 1.f, vs_new = 1.f;
  int pos_new = -1;
  if constexpr (FUSE) {
    constexpr int HALF = D / 2;
    pos_new = rp.pos[b];
    const int i0 = (dc % (LPR / 2)) * EPL;               // this lane's elements of the low half (its partner chunk: + HALF)
    const bool is_hi = dc >= LPR / 2;
    const unsigned short* row = Q + (int64_t)b * ldq + h * D;
    Wd k_row;
#pragma unroll
    for (int c = 0; c < EPL / 8; ++c) {                  // 8 elements per rope_rot8
      const int ic = i0 + 8 * c;
      const u32x4 qlo = *(const u32x4*)(row + ic), qhi = *(const u32x4*)(row + ic + HALF);
      const u32x4 klo = *(const u32x4*)(row + rp.k_off + ic), khi = *(const u32x4*)(row + rp.k_off + ic + HALF);
      const float* cp = rp.cosT + (int64_t)pos_new * HALF + ic;
      const float* sp = rp.sinT + (int64_t)pos_new * HALF + ic;
      const f32x4 c0 = *(const f32x4*)cp, c1 = *(const f32x4*)(cp + 4), s0 = *(const f32x4*)sp, s1 = *(const f32x4*)(sp + 4);
      u32x4 olo, ohi;
      rope_rot8(qlo, qhi, c0, c1, s0, s1, olo, ohi);
      const u32x4 qo = is_hi ? ohi : olo;
      rope_rot8(klo, khi, c0, c1, s0, s1, olo, ohi);
      const u32x4 ko = is_hi ? ohi : olo;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        q_raw[0][4 * c + t] = qo[t];
        k_row[4 * c + t] = ko[t];
      }
    }
    const Wd v_row = *(const Wd*)(row + rp.v_off + dc * EPL);
    if constexpr (F8) {            // every lane rounds (the row maximum is a shuffle over the row's LPR lanes)
      unsigned kx[NW], vx[NW], kq[NW / 2], vq[NW / 2];
#pragma unroll
      for (int t = 0; t < NW; ++t) {
        kx[t] = k_row[t];
        vx[t] = v_row[t];
      }
      kv_fp8_quant<LPR, NW>(kx, kq, ks_new);
      kv_fp8_quant<LPR, NW>(vx, vq, vs_new);
#pragma unroll
      for (int t = 0; t < NW / 2; ++t) {
        k_new[t] = kq[t];
        v_new[t] = vq[t];
      }
    } else {
      k_new = k_row;
      v_new = v_row;
    }
    if (wave == 0 && sub == 0 && pos_new >= 0 && pos_new < max_len) {   // one lane per chunk: the appended row
      *(Raw*)((char*)rp.kc + (base + (int64_t)pos_new * D + dc * EPL) * EB) = k_new;
      *(Raw*)((char*)rp.vc + (base + (int64_t)pos_new * D + dc * EPL) * EB) = v_new;
      if (F8 && dc == 0) {
        rp.ks[sbase + pos_new] = ks_new;
        rp.vs[sbase + pos_new] = vs_new;
      }
    }
  } else if constexpr (TILE) {
#pragma unroll
    for (int x = 0; x < NQ; ++x)
      q_raw[x] = rq[x] >= 0 ? *(const Wd*)(Q + (int64_t)rq[x] * ldq + (h * NG + x % NG) * D + dc * EPL) : Wd{};
  } else {
#pragma unroll
    for (int g = 0; g < NG; ++g) q_raw[g] = *(const Wd*)(Q + (int64_t)bq * ldq + (h * NG + g) * D + dc * EPL);
  }
  float q[NQ][EPL], m[NQ], l[NQ], o[NQ][EPL];
#pragma unroll
  for (int g = 0; g < NQ; ++g) {
#pragma unroll
    for (int t = 0; t < NW; ++t) {
      q[g][2 * t] = __uint_as_float(q_raw[g][t] << 16) * scale_log2e;
      q[g][2 * t + 1] = __uint_as_float(q_raw[g][t] & 0xffff0000u) * scale_log2e;
    }
    m[g] = NEG_BIG;
    l[g] = 0.f;
#pragma unroll
    for (int t = 0; t < EPL; ++t) o[g][t] = 0.f;
  }

  // A stream folds its keys in GROUPS of G = 4 (the same groups whatever UNR is): the four scores of a group are independent dot
  // products, ONE running-maximum update and ONE rescale serve all four, and their exponentials and the o / l updates are
  // independent again.  The per-key form was one serial chain per key — maximum, two exponentials, nine dependent FMAs — 24 links
  // deep for a 385-key prompt at one sequence per block (22 us per call at a decode batch of 1).
  constexpr int G = 4;
  static_assert(UNR % G == 0, "key rounds are consumed in groups of four");
  for (int j0 = wave * KPW; j0 < len; j0 += 4 * KPW * UNR) {
    Raw kr[UNR], vr[UNR];
    float ksr[UNR], vsr[UNR];
    unsigned sgr[UNR];                   // MASK: the keys' segment bytes
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int key = min(j0 + u * 4 * KPW + sub, len - 1);
      kr[u] = *(const Raw*)(kp + (int64_t)key * D * EB);
      vr[u] = *(const Raw*)(vp + (int64_t)key * D * EB);
      if constexpr (F8) {
        ksr[u] = Ks[sbase + key];
        vsr[u] = Vs[sbase + key];
      } else {
        ksr[u] = vsr[u] = 1.f;
      }
      if constexpr (MASK) sgr[u] = segp[key];     // (turned into the key's mask bit below, once for the NG heads)
      if (FUSE && key == pos_new) {      // the row this launch appends: from registers (the store above may not have landed)
        kr[u] = k_new;
        vr[u] = v_new;
        ksr[u] = ks_new;
        vsr[u] = vs_new;
      }
    }
    if constexpr (MASK) {
#pragma unroll
      for (int u = 0; u < UNR; ++u) sgr[u] = sgr[u] < 32u ? 1u << sgr[u] : 0u;     // ids >= 32 are never blocked
    }
#pragma unroll
    for (int gk = 0; gk < UNR / G; ++gk) {
#pragma unroll
      for (int g = 0; g < NQ; ++g) {
        if constexpr (TILE) {
          if (j0 + gk * G * 4 * KPW >= qlen[g]) continue;     // wave-uniform: every key of the group is past this state's end
        }
        float s[G];
        bool ok[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
          const int u = gk * G + i;
          const Wd kw = kv_words<F8, EPL>(kr[u], ksr[u]);
          float d = 0.f;
#pragma unroll
          for (int t = 0; t < NW; ++t) {
            d += q[g][2 * t] * __uint_as_float(kw[t] << 16);
            d += q[g][2 * t + 1] * __uint_as_float(kw[t] & 0xffff0000u);
          }
#pragma unroll
          for (int x = 1; x < LPR; x <<= 1) d += __shfl_xor(d, x, 64);
          ok[i] = j0 + u * 4 * KPW + sub < (TILE ? qlen[g] : len);
          if constexpr (MASK) ok[i] = ok[i] && !(blk[g] & sgr[u]);
          s[i] = ok[i] ? d : NEG_BIG;
        }
        const float m_new = fmaxf(fmaxf(m[g], fmaxf(s[0], s[1])), fmaxf(s[2], s[3]));
        const float alpha = __builtin_amdgcn_exp2f(m[g] - m_new);
        float pe[G];
#pragma unroll
        for (int i = 0; i < G; ++i) pe[i] = ok[i] ? __builtin_amdgcn_exp2f(s[i] - m_new) : 0.f;
        m[g] = m_new;
        l[g] = l[g] * alpha + ((pe[0] + pe[1]) + (pe[2] + pe[3]));
        Wd vw[G];
#pragma unroll
        for (int i = 0; i < G; ++i) vw[i] = kv_words<F8, EPL>(vr[gk * G + i], vsr[gk * G + i]);
#pragma unroll
        for (int t = 0; t < NW; ++t) {
          float a0 = o[g][2 * t] * alpha, a1 = o[g][2 * t + 1] * alpha;
#pragma unroll
          for (int i = 0; i < G; ++i) {
            a0 = fmaf(pe[i], __uint_as_float(vw[i][t] << 16), a0);
            a1 = fmaf(pe[i], __uint_as_float(vw[i][t] & 0xffff0000u), a1);
          }
          o[g][2 * t] = a0;
          o[g][2 * t + 1] = a1;
        }
      }
    }
  }
  const int stream = wave * KPW + sub;
#pragma unroll
  for (int g = 0; g < NQ; ++g) {       // one head (of one slot) at a time through the one merge buffer
    if (g) __syncthreads();            // the previous head's readers are done
#pragma unroll
    for (int t = 0; t < EPL; ++t) sm[stream][dc * EPL + t] = o[g][t];
    if (dc == 0) {
      sm[stream][D] = m[g];
      sm[stream][D + 1] = l[g];
    }
    __syncthreads();
    if (threadIdx.x < D) {
      const int d = threadIdx.x;
      float M = NEG_BIG;
#pragma unroll
      for (int s = 0; s < NSTREAM; ++s) M = fmaxf(M, sm[s][D]);
      float L = 0.f, acc = 0.f;
#pragma unroll
      for (int s = 0; s < NSTREAM; ++s) {
        const float w = __builtin_amdgcn_exp2f(sm[s][D] - M);
        L += sm[s][D + 1] * w;
        acc += sm[s][d] * w;
      }
      // F8: a NaN cache row (a non-finite appended k / v) makes L NaN, and the output of this (sequence, head) NaN; the bf16
      // kernel's L > 0 test would turn it into zeros.  Identical for every finite input.
      const bool live = F8 ? !(L <= 0.f) : L > 0.f;
      if constexpr (TILE) {
        if (rq[g] >= 0) O[(int64_t)rq[g] * ldo + (h * NG + g % NG) * D + d] = f32_to_bf16_bits(live ? acc / L : 0.f);
      } else {
        O[(int64_t)bq * ldo + (h * NG + g) * D + d] = f32_to_bf16_bits(live ? acc / L : 0.f);
      }
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// One call's arguments: what every form has, in the order of the kernel's list, then the kernel's own tail struct for what only
// some forms have (FORM_FUSE: cosT .. v_off, with kc / vc / ks / vs the caches again, writable; FORM_MASK: seg .. row_q; zero
// otherwise, as the kernel is handed it).
struct DecodeArgs {
  const void* Q;                // the query rows, or with FORM_FUSE the projection's q | k | v rows
  int64_t ldq;
  const void *Kc, *Vc;          // bf16 caches, or the e4m3fn byte planes
  const float *Ks, *Vs;         // FORM_F8: the scale planes; NULL otherwise
  void* O;
  int64_t ldo;
  const int32_t* lens;
  int32_t rows;                 // grid rows: n_seqs, the list entries of FORM_MASK, or the tiles of FORM_CUT
  int32_t H, Hkv, D, max_len;   // query heads, heads of the cache (= H unless FORM_GQA / FORM_MASK / FORM_CUT)
  float scale;
  void* stream;
  DecodeCut tail = {};
  int32_t tile_rows = 0;        // FORM_CUT: the slots per tile the caller built its tables for
};
// What an entry point's form has.  FORM_GQA: the entry point takes n_kv_heads (a masked call always does); FORM_EPL16: the bf16
// reference of the fp8 lane mapping; FORM_CUT: row tiles (lens is NULL: every slot brings its own key count).
enum : unsigned { FORM_F8 = 1, FORM_FUSE = 2, FORM_GQA = 4, FORM_MASK = 8, FORM_EPL16 = 16, FORM_CUT = 32 };

// Slots per tile of FORM_CUT by group size G (checked: 1..8): R * G <= 4 online-softmax states next to UNR = 4 key rounds are
// what the table above shows without scratch; from G = 3 on a tile is one row.
constexpr int cut_tile_rows(int G) { return G == 1 ? 4 : G == 2 ? 2 : 1; }

// The checks of every form, each condition once.  Which form tests what (x), G = H / Hkv:
//                                                          bf16 epl16 fp8 | rope_bf16 rope_fp8 | gqa      | masked
//   rows 1..65535, n_heads > 0, max_len > 0                  x    x    x  |    x         x     |  x       |   x
//   operands non-NULL (each form's own)                      x    x    x  |    x         x     |  x       |   x
//   head_dim 64 or 128                                       x    x    x  |    x         x     |  x       |   x
//   Hkv 1..65535 divides H, G <= 8, G > 1 only at 128        -    -    -  |    -         -     |  x       |   x
//   q | k | v blocks: k_off, v_off % 8, disjoint inside ld   -    -    -  |    x         x     |  -       |   -
//   ldq % 8, Q / Kc / Vc 16-B aligned                        x    x    x  |    x         x     |  x       |   x
//     scale planes 4-B (fp8), cos / sin 16-B (rope), blocked 4-B (masked) aligned: with the line above
//   ldq, ldo >= H * head_dim                                 -    -    -  |    -  (ldq: blocks) |  G > 1   |   x
//   ldo % 8                                                  -    -    -  |    -         -     |  G > 1   |   -
//   ld_seg >= max_len                                        -    -    -  |    -         -     |  -       |   x
//   scale finite                                             -    -    -  |    -         -     |  -       |   x
// FORM_CUT (icl_attn_cut_rows_bf16) tests what masked tests — rows = n_tiles; lens is not an operand, tile_seq and row_len are,
// head_on may be NULL — and tile_rows == cut_tile_rows(G).
// The gaps are carried over from when each form had checks of its own: no plain or fused form tests the width of O (the fused ones test that of qkv through the blocks)
// or a finite scale, none but the grouped one ldo % 8 (O is written two bytes at a time).  Closing them changes what is refused.
int attn_decode_check(const char* who, unsigned form, const DecodeArgs& a) {
  const bool f8 = form & FORM_F8, fuse = form & FORM_FUSE, gqa = form & FORM_GQA, cut = form & FORM_CUT, mask = (form & FORM_MASK) || cut;
  const DecodeCut& t = a.tail;
  const auto al = [](const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; };
  // the sizes first: an empty row list comes with NULL pointers, and is to be called an empty list
  ICL_CHECK_ARG(a.rows > 0 && a.rows <= 65535 && a.H > 0 && a.max_len > 0, "%s: bad sizes: %s=%d (1..65535), n_heads=%d, max_len=%d", who,
                cut ? "n_tiles" : mask ? "n_rows" : "n_seqs", a.rows, a.H, a.max_len);
  ICL_CHECK_ARG(a.Q && a.Kc && a.Vc && a.O && (cut || a.lens) && (!f8 || (a.Ks && a.Vs)) && (!fuse || (t.cosT && t.sinT && t.pos)) &&
                    (!mask || (t.seg && t.blocked && t.row_q)) && (!mask || cut || t.row_seq) && (!cut || (t.tile_seq && t.row_len)),
                "%s: NULL pointer", who);
  ICL_CHECK_ARG(a.D == 64 || a.D == 128, "%s: head_dim=%d (only 64 and 128)", who, a.D);
  if (gqa || mask) {
    ICL_CHECK_ARG(a.Hkv > 0 && a.Hkv <= 65535 && a.H % a.Hkv == 0, "%s: n_heads=%d is not a multiple of n_kv_heads=%d", who, a.H, a.Hkv);
    ICL_CHECK_ARG(a.H / a.Hkv <= 8, "%s: %d query heads per K/V head (G at most 8)", who, a.H / a.Hkv);
    ICL_CHECK_ARG(a.H == a.Hkv || a.D == 128, "%s: head_dim=%d (grouped-query attention: only 128)", who, a.D);
  }
  if (cut)
    ICL_CHECK_ARG(a.tile_rows == cut_tile_rows(a.H / a.Hkv), "%s: tile_rows=%d, the form's tiles hold %d rows (icl_attn_cut_tile_rows)", who,
                  a.tile_rows, cut_tile_rows(a.H / a.Hkv));
  const int64_t cols = (int64_t)a.H * a.D;
  const bool grouped = gqa && a.H > a.Hkv;      // through the grouped entry point, G = 1 is the multi-head form under its conditions
  if (fuse)
    ICL_CHECK_ARG(t.k_off % 8 == 0 && t.v_off % 8 == 0 && t.k_off >= cols && t.v_off >= t.k_off + cols && a.ldq >= t.v_off + cols,
                  "%s: q | k | v column blocks must be 8-element aligned and disjoint inside a row", who);
  ICL_CHECK_ARG(a.ldq % 8 == 0 && al(a.Q, 16) && al(a.Kc, 16) && al(a.Vc, 16) && (!f8 || (al(a.Ks, 4) && al(a.Vs, 4))) &&
                    (!fuse || (al(t.cosT, 16) && al(t.sinT, 16))) && (!mask || al(t.blocked, 4)), "%s: misaligned operands", who);
  if (mask || grouped)
    ICL_CHECK_ARG(a.ldq >= cols && a.ldo >= cols, "%s: ldq=%lld / ldo=%lld must hold n_heads * head_dim = %lld columns", who,
                  (long long)a.ldq, (long long)a.ldo, (long long)cols);
  if (grouped) ICL_CHECK_ARG(a.ldo % 8 == 0, "%s: ldo=%lld must be a multiple of 8", who, (long long)a.ldo);
  if (mask) {
    ICL_CHECK_ARG(t.ld_seg >= a.max_len, "%s: ld_seg=%lld < max_len=%d", who, (long long)t.ld_seg, a.max_len);
    ICL_CHECK_ARG(__builtin_isfinite(a.scale), "%s: scale is not finite", who);
  }
  return ICL_OK;
}

// One workgroup per (head of the cache, row).  The kernel's argument list, and for an unmasked form the DecodeRope part of the tail.
template <int D, int UNR, bool FUSE, bool F8, int EPL, int NG, bool MASK, int R = 0>
void attn_decode_launch(const DecodeArgs& a) {
  const typename DecodeTail<MASK, R>::T tail = a.tail;
  hipLaunchKernelGGL((attn_decode_kernel<D, UNR, FUSE, F8, EPL, NG, MASK, R>), dim3(a.Hkv, a.rows), dim3(256), 0, (hipStream_t)a.stream,
                     (const unsigned short*)a.Q, a.ldq, a.Kc, a.Vc, a.Ks, a.Vs, (unsigned short*)a.O, a.ldo, a.lens, a.Hkv, a.max_len,
                     a.scale * LOG2E, tail);
}

// Multi-head, UNR by the grid: few workgroups (at most four per CU: latency-bound, not bandwidth-bound) take 16 key rounds at 8
// elements per lane and 8 at 16 (the same keys in flight per loop iteration), a full chip 4.  MASK: 8 whatever the grid.
template <bool FUSE, bool F8, int EPL, bool MASK = false>
void attn_decode_mha(const DecodeArgs& a) {
  constexpr int UFEW = MASK || EPL == 16 ? 8 : 16, UMANY = MASK ? 8 : 4;
  const bool few = (int64_t)a.rows * a.Hkv <= 1024;
  if (a.D == 64) few ? attn_decode_launch<64, UFEW, FUSE, F8, EPL, 1, MASK>(a) : attn_decode_launch<64, UMANY, FUSE, F8, EPL, 1, MASK>(a);
  else few ? attn_decode_launch<128, UFEW, FUSE, F8, EPL, 1, MASK>(a) : attn_decode_launch<128, UMANY, FUSE, F8, EPL, 1, MASK>(a);
}

// Grouped-query, G = 2 .. 8 (checked): key rounds in flight per group size, 8 (64 VGPRs of loads) next to two heads of state, 4
// from three heads on.  Masked and unmasked share the table.
template <bool MASK>
void attn_decode_gqa(int G, const DecodeArgs& a) {
  switch (G) {
    case 2: return attn_decode_launch<128, 8, false, false, 8, 2, MASK>(a);
    case 3: return attn_decode_launch<128, 4, false, false, 8, 3, MASK>(a);
    case 4: return attn_decode_launch<128, 4, false, false, 8, 4, MASK>(a);
    case 5: return attn_decode_launch<128, 4, false, false, 8, 5, MASK>(a);
    case 6: return attn_decode_launch<128, 4, false, false, 8, 6, MASK>(a);
    case 7: return attn_decode_launch<128, 4, false, false, 8, 7, MASK>(a);
    case 8: return attn_decode_launch<128, 4, false, false, 8, 8, MASK>(a);
  }
}

// Row tiles (FORM_CUT): one workgroup per (K/V head, tile), ONE instantiation per (head_dim, G) whatever the grid — R =
// cut_tile_rows(G) slots, UNR 4: the grouped table's for R * G = 3 .. 8 states.
void attn_decode_cut(int G, const DecodeArgs& a) {
  switch (G) {
    case 1: return a.D == 64 ? attn_decode_launch<64, 4, false, false, 8, 1, true, cut_tile_rows(1)>(a)
                             : attn_decode_launch<128, 4, false, false, 8, 1, true, cut_tile_rows(1)>(a);
    case 2: return attn_decode_launch<128, 4, false, false, 8, 2, true, cut_tile_rows(2)>(a);
    case 3: return attn_decode_launch<128, 4, false, false, 8, 3, true, 1>(a);
    case 4: return attn_decode_launch<128, 4, false, false, 8, 4, true, 1>(a);
    case 5: return attn_decode_launch<128, 4, false, false, 8, 5, true, 1>(a);
    case 6: return attn_decode_launch<128, 4, false, false, 8, 6, true, 1>(a);
    case 7: return attn_decode_launch<128, 4, false, false, 8, 7, true, 1>(a);
    case 8: return attn_decode_launch<128, 4, false, false, 8, 8, true, 1>(a);
  }
}

// The one way from an entry point to the kernel: check, pick the instantiation <D, UNR, FUSE, F8, EPL, NG, MASK, R>, launch.
int attn_decode_run(const char* who, unsigned form, const DecodeArgs& a) {
  if (const int rc = attn_decode_check(who, form, a)) return rc;
  const int G = a.H / a.Hkv;
  const bool fuse = form & FORM_FUSE;
  if (form & FORM_CUT) attn_decode_cut(G, a);
  else if (form & FORM_MASK) G > 1 ? attn_decode_gqa<true>(G, a) : attn_decode_mha<false, false, 8, true>(a);
  else if (G > 1) attn_decode_gqa<false>(G, a);
  else if (form & FORM_F8) fuse ? attn_decode_mha<true, true, 16>(a) : attn_decode_mha<false, true, 16>(a);
  else if (form & FORM_EPL16) attn_decode_mha<false, false, 16>(a);
  else fuse ? attn_decode_mha<true, false, 8>(a) : attn_decode_mha<false, false, 8>(a);
  ICL_CHECK_LAUNCH(who);
  return ICL_OK;
}

}  // namespace

extern "C" int icl_attn_decode_bf16(const void* Q, int64_t ldq, const void* Kc, const void* Vc, void* O,
                                    int64_t ldo, const int32_t* lens, int32_t n_seqs, int32_t n_heads,
                                    int32_t head_dim, int32_t max_len, float scale, void* stream) {
  return attn_decode_run("icl_attn_decode_bf16", 0,
                         {Q, ldq, Kc, Vc, nullptr, nullptr, O, ldo, lens, n_seqs, n_heads, n_heads, head_dim, max_len, scale, stream});
}

extern "C" int icl_attn_decode_bf16_epl16(const void* Q, int64_t ldq, const void* Kc, const void* Vc, void* O,
                                          int64_t ldo, const int32_t* lens, int32_t n_seqs, int32_t n_heads,
                                          int32_t head_dim, int32_t max_len, float scale, void* stream) {
  return attn_decode_run("icl_attn_decode_bf16_epl16", FORM_EPL16,
                         {Q, ldq, Kc, Vc, nullptr, nullptr, O, ldo, lens, n_seqs, n_heads, n_heads, head_dim, max_len, scale, stream});
}

extern "C" int icl_attn_decode_fp8(const void* Q, int64_t ldq, const void* Kc, const void* Vc, const float* kscale,
                                   const float* vscale, void* O, int64_t ldo, const int32_t* lens, int32_t n_seqs, int32_t n_heads,
                                   int32_t head_dim, int32_t max_len, float scale, void* stream) {
  return attn_decode_run("icl_attn_decode_fp8", FORM_F8,
                         {Q, ldq, Kc, Vc, kscale, vscale, O, ldo, lens, n_seqs, n_heads, n_heads, head_dim, max_len, scale, stream});
}

extern "C" int icl_attn_decode_gqa_bf16(const void* Q, int64_t ldq, const void* Kc, const void* Vc, void* O, int64_t ldo,
                                        const int32_t* lens, int32_t n_seqs, int32_t n_heads, int32_t n_kv_heads,
                                        int32_t head_dim, int32_t max_len, float scale, void* stream) {
  return attn_decode_run("icl_attn_decode_gqa_bf16", FORM_GQA,
                         {Q, ldq, Kc, Vc, nullptr, nullptr, O, ldo, lens, n_seqs, n_heads, n_kv_heads, head_dim, max_len, scale, stream});
}

// The masked form (attention knockout): the bf16 kernel over a row list, every key under its head's segment mask.
// n_kv_heads = 0: n_heads.
extern "C" int icl_attn_decode_masked_bf16(const void* Q, int64_t ldq, const void* Kc, const void* Vc, void* O, int64_t ldo,
                                           const int32_t* lens, const uint8_t* seg, int64_t ld_seg, const uint32_t* blocked,
                                           const int32_t* row_seq, const int32_t* row_q, int32_t n_rows, int32_t n_heads,
                                           int32_t n_kv_heads, int32_t head_dim, int32_t max_len, float scale, void* stream) {
  DecodeArgs a = {Q, ldq, Kc, Vc, nullptr, nullptr, O, ldo, lens, n_rows, n_heads, n_kv_heads ? n_kv_heads : n_heads, head_dim, max_len,
                  scale, stream};
  a.tail = {{{}, seg, ld_seg, blocked, row_seq, row_q}};
  return attn_decode_run("icl_attn_decode_masked_bf16", FORM_MASK, a);
}

// Attention cuts: the masked kernel over TILES of listed rows of one cache sequence, every slot under its own key count and mask.
extern "C" int icl_attn_cut_tile_rows(int32_t n_heads, int32_t n_kv_heads, int32_t head_dim) {
  const int Hkv = n_kv_heads ? n_kv_heads : n_heads;
  if (n_heads <= 0 || Hkv <= 0 || n_heads % Hkv || n_heads / Hkv > 8 || (head_dim != 64 && head_dim != 128) ||
      (n_heads != Hkv && head_dim != 128))
    return -1;
  return cut_tile_rows(n_heads / Hkv);
}

extern "C" int icl_attn_cut_rows_bf16(const void* Q, int64_t ldq, const void* Kc, const void* Vc, void* O, int64_t ldo,
                                      const uint8_t* seg, int64_t ld_seg, const int32_t* tile_seq, const int32_t* row_q,
                                      const int32_t* row_len, const uint32_t* blocked, const uint8_t* head_on, int32_t n_tiles,
                                      int32_t tile_rows, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, int32_t max_len,
                                      float scale, void* stream) {
  DecodeArgs a = {Q, ldq, Kc, Vc, nullptr, nullptr, O, ldo, nullptr, n_tiles, n_heads, n_kv_heads ? n_kv_heads : n_heads, head_dim,
                  max_len, scale, stream};
  a.tail = {{{}, seg, ld_seg, blocked, nullptr, row_q}, tile_seq, row_len, head_on};
  a.tile_rows = tile_rows;
  return attn_decode_run("icl_attn_cut_rows_bf16", FORM_CUT, a);
}

// The RoPE-fused forms: the tail names the caches again, writable, for the appended row.
extern "C" int icl_attn_decode_rope_bf16(const void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const float* cosT,
                                         const float* sinT, const int32_t* pos, const int32_t* seq_ids, void* kc, void* vc,
                                         void* O, int64_t ldo, const int32_t* lens, int32_t n_seqs, int32_t n_heads,
                                         int32_t head_dim, int32_t max_len, float scale, void* stream) {
  DecodeArgs a = {qkv, ld, kc, vc, nullptr, nullptr, O, ldo, lens, n_seqs, n_heads, n_heads, head_dim, max_len, scale, stream};
  a.tail = {{{cosT, sinT, pos, seq_ids, kc, vc, nullptr, nullptr, k_off, v_off}}};
  return attn_decode_run("icl_attn_decode_rope_bf16", FORM_FUSE, a);
}

extern "C" int icl_attn_decode_rope_fp8(const void* qkv, int64_t ld, int64_t k_off, int64_t v_off, const float* cosT,
                                        const float* sinT, const int32_t* pos, const int32_t* seq_ids, void* kc, void* vc,
                                        float* kscale, float* vscale, void* O, int64_t ldo, const int32_t* lens, int32_t n_seqs,
                                        int32_t n_heads, int32_t head_dim, int32_t max_len, float scale, void* stream) {
  DecodeArgs a = {qkv, ld, kc, vc, kscale, vscale, O, ldo, lens, n_seqs, n_heads, n_heads, head_dim, max_len, scale, stream};
  a.tail = {{{cosT, sinT, pos, seq_ids, kc, vc, kscale, vscale, k_off, v_off}}};
  return attn_decode_run("icl_attn_decode_rope_fp8", FORM_FUSE | FORM_F8, a);
}

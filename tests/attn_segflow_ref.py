"""The float64 reference of icl_attn_segflow_bf16 (the segment-to-segment attention flow), its per-element bound, the cases and
probes of tests/test_gpu_attn_segflow.py, deliberately wrong references (mutants) and an f32 emulation in the kernel's order.  Plain
torch on the CPU; tests/test_attn_segflow_ref.py shows without a GPU that the bound admits the emulation and rejects every mutant.

Definition (include/icl_hip.h): p(i, j) = softmax over j <= i of scale * q_i . k_j,
flow[a, c] = sum_{i < len, seg_i = a} sum_{j <= i, seg_j = c} p(i, j); an id >= n_seg on a query row: the row is summed nowhere; on
a key: counted in no segment, still in the row's denominator.

The bound, per element, against this reference on the same bf16 q and cache (the constants of tests/attn_segmass_ref.py: u = 2^-24,
C1 = 4, C2 = 2, T = 2^-126; n = len, n_c = keys of segment c, n_a = rows of segment a, S = max over the sequence's (i, j <= i) of
scale * sum_d |q_id| |k_jd|, N_ac = the number of counted (i, j) pairs):

    |flow[a, c] - ref| <= ref * (C1 * D * u * S + C2 * (n + n_c + n_a + 8) * u + 2^-17) + 2 * N_ac * T

Derivation.  (1)-(3) are the readout's (tests/attn_segmass_ref.py), per query row: a score is an f32 dot product of D exact bf16
products, a weight is a ratio in which a common shift cancels — C1 * D * u * S relative; the exponentials, the running-maximum
rescales, the f32 row sum over at most n keys and the division — C2 * (n + 8) * u; the f32 sum of a row's at most n_c weights of
segment c (inside the MFMA and across tiles) — C2 * n_c * u.  Every row of the sequence is held to the sequence's S and n (a row
has i + 1 <= n keys).  (4) New: the weights enter the segment product as hi + lo, hi = bf16_rne(p), lo = bf16_rne(p - hi).  p - hi is
exact in f32 (|p - hi| <= 2^-9 p, a multiple of ulp(p) / 2^k that fits 24 bits), so |p - hi - lo| <= 2^-9 * 2^-9 p = 2^-18 p; the
one-hot operand is exact.  Taken as 2^-17.  (5) New: flow[a, c] is an f32 sum over the n_a rows of segment a, in position order
within a wave and over four wave accumulators: at most (n_a + 3) * u relative to the sum — C2 * n_a * u.  Every summand is
non-negative, so the relative errors of the summands carry to the sums.  (6) The absolute term: an exponential below T = 2^-126 is
flushed or rounded on the subnormal grid, and a subnormal hi or lo operand may be flushed by the MFMA: at most 2 T per counted weight
(hi and lo), the division by l >= 1 does not enlarge it: 2 * N_ac * T.  With N_ac = 0 the reference is 0 and so is the bound: a pair
with nothing to count is exactly 0.0.  The bound is derived, not tuned; the largest err / bound per form is printed by the GPU test.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

import attn_segmass_ref as sr

U, C1, C2, TINY, IGNORE, W_EXACT = sr.U, sr.C1, sr.C2, sr.TINY, sr.IGNORE, sr.W_EXACT
SPLIT = 2.0 ** -17

LENS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 385)      # every boundary of the 32-query block, the 128-query pass, the 64-key tile
MAX_LEN = 448
SEED = 5531
FORMS = ((64, 3, 3), (128, 4, 4), (128, 4, 2), (128, 8, 1))          # (D, n_heads, n_kv_heads)
CASES = [(D, H, Hkv, n_seg) for D, H, Hkv in FORMS for n_seg in (1, 2, 32)]
REF_MUTANTS = ("causal_strict", "key_plus1", "len_plus1", "transposed", "ignored_q_into_0", "ignored_k_into_0", "natural_k_order")
# position x = 8 * half + j of a 16-key k-step holds key offset 8 * (j >> 2) + 4 * half + (j & 3): the accumulator's register order
K_PERM = tuple(8 * ((x & 7) >> 2) + 4 * (x >> 3) + (x & 3) for x in range(16))


def case_id(case):
    D, H, Hkv, n_seg = case
    return f"D{D}-H{H}-kv{Hkv}-seg{n_seg}"


def cu_of(lens):
    cu = [0]
    for L in lens:
        cu.append(cu[-1] + int(L))
    return cu


# ------------------------------------------------------------------------------------------------------------------
# inputs: q packed bf16 [sum lens, H * D], K cache bf16 [B, Hkv, max_len, D] with NaN at and past each length
# ------------------------------------------------------------------------------------------------------------------
def make_seg(lens, n_seg, max_len=MAX_LEN):
    return sr.make_seg(lens, n_seg, max_len=max_len, seed=SEED)


def _nan_tail(kc, lens):
    for b, L in enumerate(lens):
        kc[b, :, L:] = float("nan")
    return kc


def random_case(lens, H, Hkv, D, max_len=MAX_LEN, seed=SEED):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(sum(lens), H * D, generator=g).to(torch.bfloat16)
    kc = torch.randn(len(lens), Hkv, max_len, D, generator=g).to(torch.bfloat16)
    return q, _nan_tail(kc, lens)


def count_probe(lens, H, Hkv, D, max_len=MAX_LEN, seed=SEED):
    """All keys of a (sequence, K/V head) equal: every score of a row has the same bits, p(i, j) = 1 / (i + 1)."""
    g = torch.Generator().manual_seed(seed + 1)
    q = torch.randn(sum(lens), H * D, generator=g).to(torch.bfloat16)
    row = torch.randn(len(lens), Hkv, 1, D, generator=g).to(torch.bfloat16)
    return q, _nan_tail(row.expand(-1, -1, max_len, -1).clone(), lens)


def count_flow(lens, seg, n_seg):
    """The count probe's flow as exact rationals in float64, [B, n_seg, n_seg], and the ignored keys' share per query segment
    [B, n_seg]: sum_c flow[a, c] + ignored[a] = rows[a]."""
    flow = torch.zeros(len(lens), n_seg, n_seg, dtype=torch.float64)
    ign = torch.zeros(len(lens), n_seg, dtype=torch.float64)
    for b, L in enumerate(lens):
        ids = seg[b, :L].long()
        onehot = torch.zeros(L, n_seg + 1, dtype=torch.float64)
        onehot[torch.arange(L), ids.clamp(max=n_seg)] = 1.0
        share = onehot.cumsum(0) / torch.arange(1, L + 1, dtype=torch.float64)[:, None]      # [i, c]: keys j <= i of segment c / (i + 1)
        for a in range(n_seg):
            sel = ids == a
            flow[b, a] = share[sel, :n_seg].sum(0)
            ign[b, a] = share[sel, n_seg].sum()
    return flow, ign


def peak_probe(lens, H, Hkv, D, seg, n_seg, max_len=MAX_LEN, seed=SEED):
    """``attn_segmass_ref.peak_probe`` per query row: K rows are +-1 patterns, the query of row i and head h is 8 x the pattern of
    its target key among the keys 0 .. i (target kind h mod 4 of ``peak_targets`` on that prefix)."""
    g = torch.Generator().manual_seed(seed + 2)
    kc = (torch.randint(0, 2, (len(lens), Hkv, max_len, D), generator=g) * 2 - 1).float()
    q = torch.zeros(sum(lens), H, D)
    G, cu = H // Hkv, cu_of(lens)
    for b, L in enumerate(lens):
        for i in range(L):
            t = sr.peak_targets(seg[b], i + 1, n_seg)
            for h in range(H):
                q[cu[b] + i, h] = 8 * kc[b, h // G, t[h % 4]]
    return q.reshape(-1, H * D).to(torch.bfloat16), _nan_tail(kc.to(torch.bfloat16), lens)


def single_case(D=128, H=2, n=32, seed=SEED):
    """Segments that hold single keys and single rows: one sequence of n <= 32 positions, seg[i] = i — flow[a, c] is the single
    weight p(a, c), nothing averages a rounding of P."""
    g = torch.Generator().manual_seed(seed + 3)
    q = torch.randn(n, H * D, generator=g).to(torch.bfloat16)
    kc = torch.randn(1, H, 64, D, generator=g).to(torch.bfloat16)
    seg = torch.full((1, 64), 0xFF, dtype=torch.uint8)
    seg[0, :n] = torch.arange(n, dtype=torch.uint8)
    return q, _nan_tail(kc, [n]), seg


# ------------------------------------------------------------------------------------------------------------------
# the reference and its mutants
# ------------------------------------------------------------------------------------------------------------------
@dataclass
class Ref:
    flow: torch.Tensor       # f64 [B, H, n_seg, n_seg]
    S: torch.Tensor          # f64 [B, H]
    n: torch.Tensor          # f64 [B]
    n_c: torch.Tensor        # f64 [B, n_seg]: keys of segment c
    n_a: torch.Tensor        # f64 [B, n_seg]: rows of segment a (the same counts: a position is a row and a key)
    N_ac: torch.Tensor       # f64 [B, n_seg, n_seg]: counted (i, j) pairs
    rows: torch.Tensor       # int64 [B, n_seg]
    pmax_min: float          # the smallest, over all rows and heads, of the row's largest weight


def reference(q, kc, lens, seg, n_seg, H, Hkv, D, scale, mutate=None) -> Ref:
    """float64, on the bf16 values given.  ``mutate``: one of REF_MUTANTS — causal_strict (j < i; row 0 sees nothing), key_plus1
    (key i + 1 admitted), len_plus1 (the sequence is one position longer: its last position, query, key and id, once more),
    transposed (the query's segment taken from the key), ignored_q_into_0 / ignored_k_into_0 (ignored ids on query rows / keys count
    as segment 0), natural_k_order (the weight of the key at register position x of a 16-key group is credited to the key at
    natural position x)."""
    assert mutate is None or mutate in REF_MUTANTS
    Bn, G, cu = len(lens), H // Hkv, cu_of(lens)
    flow = torch.zeros(Bn, H, n_seg, n_seg, dtype=torch.float64)
    S, n = torch.zeros(Bn, H, dtype=torch.float64), torch.zeros(Bn, dtype=torch.float64)
    n_c, N_ac = torch.zeros(Bn, n_seg, dtype=torch.float64), torch.zeros(Bn, n_seg, n_seg, dtype=torch.float64)
    pmax_min = 1.0
    for b, L in enumerate(lens):
        L = int(L)
        k = kc[b, :, :L].double().repeat_interleave(G, 0)                        # [H, L, D]
        qh = q[cu[b]:cu[b] + L].double().reshape(L, H, D).transpose(0, 1)        # [H, L, D]
        ids = seg[b, :L].long().clone()
        n[b] = L
        oh = torch.zeros(L, n_seg + 1, dtype=torch.float64)
        oh[torch.arange(L), ids.clamp(max=n_seg)] = 1.0
        oh = oh[:, :n_seg]
        tril = torch.ones(L, L, dtype=torch.float64).tril()
        n_c[b] = oh.sum(0)
        N_ac[b] = oh.T @ tril @ oh
        S[b] = (abs(scale) * torch.einsum("hid,hjd->hij", qh.abs(), k.abs()) * tril).amax((1, 2))
        if mutate == "len_plus1":
            k, qh, ids, L = torch.cat([k, k[:, -1:]], 1), torch.cat([qh, qh[:, -1:]], 1), torch.cat([ids, ids[-1:]]), L + 1
        s = scale * torch.einsum("hid,hjd->hij", qh, k)
        vis = torch.ones(L, L, dtype=torch.bool).tril(-1 if mutate == "causal_strict" else 1 if mutate == "key_plus1" else 0)
        s = s.masked_fill(~vis, float("-inf"))
        e = torch.exp(s - s.amax(-1, keepdim=True).clamp_min(-1e300))
        e = torch.where(vis, e, torch.zeros_like(e))
        p = e / e.sum(-1, keepdim=True).clamp_min(1e-300)                        # a row without a key: zeros
        if mutate is None:
            pmax_min = min(pmax_min, float(p.amax(-1).min()))
        qi, ki = ids.clone(), ids.clone()
        if mutate == "ignored_q_into_0":
            qi[qi >= n_seg] = 0
        if mutate == "ignored_k_into_0":
            ki[ki >= n_seg] = 0
        if mutate == "natural_k_order":
            full = seg[b].long()
            credit = torch.tensor([16 * (j // 16) + K_PERM.index(j % 16) for j in range(L)])     # key j sits at register position x
            ki = full[credit]
        ohq, ohk = torch.zeros(L, n_seg + 1, dtype=torch.float64), torch.zeros(L, n_seg + 1, dtype=torch.float64)
        ohq[torch.arange(L), qi.clamp(max=n_seg)] = 1.0
        ohk[torch.arange(L), ki.clamp(max=n_seg)] = 1.0
        f = torch.einsum("ia,hij,jc->hac", ohq[:, :n_seg], p, ohk[:, :n_seg])
        flow[b] = f.transpose(1, 2) if mutate == "transposed" else f
    return Ref(flow, S, n, n_c, n_c.clone(), N_ac, n_c.long(), pmax_min)


def _bf16(x):
    return x.to(torch.bfloat16).float()


def emulate_f32(q, kc, lens, seg, n_seg, H, Hkv, D, scale, hi_only=False, natural_k_order=False):
    """f32, in the kernel's order: a wave's 32 query rows at a time through the 64-key tiles their block sees, base-2 logits, online
    (m, l) with the row sum split over the lane's two halves, the weights as hi + lo (``hi_only``: rounded once), the segment sums
    per 16-key step in key order (hi, then lo), the rescale per tile, the division by l, then the rows into their segment's row of
    the wave's accumulator in position order, the four wave accumulators merged in wave order.  -> f32 [B, H, n_seg, n_seg]"""
    LOG2E = torch.tensor(1.4426950408889634, dtype=torch.float32)
    sl = (torch.tensor(scale, dtype=torch.float32) * LOG2E)
    Bn, G, cu = len(lens), H // Hkv, cu_of(lens)
    out = torch.zeros(Bn, H, n_seg, n_seg, dtype=torch.float32)
    half = torch.tensor([(j >> 2) & 1 for j in range(64)])                       # which half of the wave holds key offset j
    order = torch.tensor([x for hh in range(2) for x in range(64) if ((x >> 2) & 1) == hh])      # a half's keys in register order
    for b, L in enumerate(lens):
        ids = seg[b, :L].long()
        E = torch.zeros(((L + 63) // 64) * 64, 32, dtype=torch.float32)          # one-hot [key][segment]; ids >= 32 nowhere
        for j in range(L):
            src = 16 * (j // 16) + K_PERM.index(j % 16) if natural_k_order else j  # whose id the operand holds at key j's position
            sid = int(seg[b, src]) if src < seg.shape[1] else 255
            if sid < 32 and src < L:
                E[j, sid] = 1.0
        for h in range(H):
            kf = kc[b, h // G, :L].float()
            qf = q[cu[b]:cu[b] + L, h * D:(h + 1) * D].float()
            acc = torch.zeros(4, 32, 32, dtype=torch.float32)
            for qw in range(0, L, 32):
                wave, rows = (qw // 32) % 4, min(32, L - qw)
                qpos = torch.arange(qw, qw + rows)
                m = torch.full((rows,), -1.0e30, dtype=torch.float32)
                l2 = torch.zeros(rows, 2, dtype=torch.float32)
                F = torch.zeros(rows, 32, dtype=torch.float32)
                for k0 in range(0, min(L, qw + 32), 64):
                    kt = kf[k0:k0 + 64]
                    nk = kt.shape[0]
                    s = (qf[qw:qw + rows] @ kt.T) * sl
                    key = torch.arange(k0, k0 + nk)
                    ok = key[None, :] <= qpos[:, None]
                    s = torch.where(ok, s, torch.full_like(s, -1.0e30))
                    m_new = torch.maximum(m, s.amax(1))
                    alpha = torch.exp2(m - m_new)
                    e = torch.where(ok, torch.exp2(s - m_new[:, None]), torch.zeros_like(s))
                    ep = torch.zeros(rows, 64, dtype=torch.float32)
                    ep[:, :nk] = e
                    psum = torch.stack([ep[:, order[:32]].cumsum(1)[:, -1], ep[:, order[32:]].cumsum(1)[:, -1]], 1)
                    l2 = l2 * alpha[:, None] + psum
                    m = m_new
                    hi = _bf16(ep)
                    lo = torch.zeros_like(hi) if hi_only else _bf16(ep - hi)
                    F = F * alpha[:, None]
                    Et = E[k0:k0 + 64]
                    for s16 in range(0, 64, 16):
                        for part in (hi, lo):
                            terms = part[:, s16:s16 + 16, None] * Et[None, s16:s16 + 16, :]      # [rows, 16, 32]
                            F = torch.cat([F[:, None, :], terms], 1).cumsum(1)[:, -1]
                F = F * (1.0 / (l2[:, 0] + l2[:, 1]))[:, None]
                for r in range(rows):
                    a = int(ids[qw + r])
                    if a < n_seg:
                        acc[wave, a] += F[r]
            tot = ((acc[0] + acc[1]) + acc[2]) + acc[3]
            out[b, h] = tot[:n_seg, :n_seg]
    return out


# ------------------------------------------------------------------------------------------------------------------
# the bound
# ------------------------------------------------------------------------------------------------------------------
def flow_ratio(got, R: Ref, D):
    """err / bound per element of flow, [B, H, n_seg, n_seg] (inf for a non-finite value or any error where the bound is 0)."""
    rel = (C1 * D * U * R.S[:, :, None, None] +
           C2 * (R.n[:, None, None, None] + R.n_c[:, None, None, :] + R.n_a[:, None, :, None] + 8) * U + SPLIT)
    bound = R.flow * rel + 2 * R.N_ac[:, None] * TINY
    return sr._ratio((got.double() - R.flow).abs(), bound)


def worst(got, R: Ref, D):
    return float(flow_ratio(got, R, D).max())


def describe(ratio):
    idx = torch.nonzero(ratio > 1)
    return "none" if idx.numel() == 0 else f"{idx.shape[0]} elements; first at (sequence, head, a, c) {tuple(int(x) for x in idx[0])}"

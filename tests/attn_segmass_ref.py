"""The float64 reference of icl_attn_segmass_bf16 (the prompt-attention readout), its per-element bound, the cases and probes of
tests/test_gpu_attn_segmass.py, deliberately wrong references (mutants) and an f32 emulation of the definition.  Plain torch / numpy
on the CPU; tests/test_attn_segmass_ref.py shows without a GPU that the bound admits the emulation and rejects every mutant.

Definition (include/icl_hip.h): s_j = scale * sum_d q_d k_jd, p_j = exp(s_j - max s) / sum_i exp(s_i - max s),
mass_g = sum_{j < len, seg_j = g} p_j.

The bound, per element, against this reference on the same bf16 q and cache (u = 2^-24, C_DOT = 2, c1 = 4, c2 = 2: the constants of
tests/test_gpu_attention_exact.py; n = lens[b], n_g = keys of segment g, S = max_j scale * sum_d |q_d| |k_jd|, T = 2^-126):

    |probs_j - ref_j| <= ref_j * (c1 * D * u * S + c2 * (n + 8) * u) + T
    |mass_g  - ref_g| <= ref_g * (c1 * D * u * S + c2 * (n + n_g + 8) * u) + n_g * T

Derivation.  (1) A score is an f32 dot product of D exact bf16 products, with q scaled by scale * log2(e) once per element:
|ds_j| <= C_DOT * D * u * S.  A weight is a ratio e_j / sum e in which a common shift cancels, so to first order
|dp_j| / p_j <= |ds_j| + max_k |ds_k| <= 2 * C_DOT * D * u * S = c1 * D * u * S.  (2) The hardware exponential is good to one ulp,
the running-maximum rescales multiply by exponentials of the same kind, the sum of the e_j over n keys is an f32 accumulation
(C_DOT * n * u relative: all terms are positive) and one division ends it: c2 * (n + 8) * u with c2 = C_DOT.  (3) A segment's mass
is an f32 sum of its n_g non-negative weights in key order: at most n_g * u relative to the sum, taken as c2 * n_g * u — the n_g
term.  Each p_j carries the relative error of (1) + (2), and so does their sum.  (4) What a relative bound lacks: f32 has no
relative precision below its smallest normal number T = 2^-126.  An exponential below T is flushed to zero or rounded on the
subnormal grid, and the division by sum e >= 1 does not enlarge that: an absolute T per weight, n_g * T per segment.  It matters only
where a weight is below 1e-37 (the peak probe's far keys), and leaves "a segment without a key is exactly 0" intact: n_g = 0 and
ref = 0 give a bound of 0.  The bound is derived, not tuned; the largest err / bound per form is printed by the GPU test.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

U = 2.0 ** -24
C1 = 4
C2 = 2
TINY = 2.0 ** -126
W_EXACT = 1.0 - 2.0 ** -12
IGNORE = 255

LENS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 385)
MAX_LEN = 448
SEED = 4421
MUTANTS = ("drop_key", "dup_last", "lens_minus1", "move_boundary", "ignored_into_0")
SEG_MUTANTS = ("move_boundary", "ignored_into_0")

# (D, n_heads, n_kv_heads, n_seg): multi-head at D 64 / 128 and H 3 / 4 with 1, 2 and 32 segments; grouped at D 128, G in 2, 4, 7, 8
CASES = ([(D, H, H, n_seg) for D in (64, 128) for H in (3, 4) for n_seg in (1, 2, 32)] +
         [(128, 2 * G, 2, n_seg) for G in (2, 4, 7, 8) for n_seg in (2, 32)] + [(128, 4, 2, 1)])


def case_id(case):
    D, H, Hkv, n_seg = case
    return f"D{D}-H{H}-kv{Hkv}-seg{n_seg}"


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
def make_seg(lens, n_seg, max_len=MAX_LEN, seed=SEED):
    """uint8 [len(lens), max_len]: per row, contiguous runs of non-decreasing ids below n_seg; with n_seg >= 3 id 1 is never used (an
    empty segment in every row), with n_seg == 2 every third row uses id 0 only; in rows of >= 3 keys every fifth position or so
    (never key 0) carries an ignored id (n_seg, 200 or 255).  Bytes at or past the length are 0xFF."""
    g = np.random.default_rng(seed + n_seg)
    seg = np.full((len(lens), max_len), 0xFF, dtype=np.uint8)
    for b, L in enumerate(lens):
        ids = np.sort(g.integers(0, n_seg, L))
        if n_seg >= 3:
            ids[ids == 1] = 2
        if n_seg == 2 and b % 3 == 0:
            ids[:] = 0
        if L >= 3:
            for j in range(1, L):
                if (7 * j + b) % 5 == 0:
                    ids[j] = (n_seg, 200, IGNORE)[j % 3]
        seg[b, :L] = ids
    return torch.from_numpy(seg)


def random_case(lens, H, Hkv, D, max_len=MAX_LEN, seed=SEED):
    """i.i.d. normal bf16 q [B, H * D] and K cache [B, Hkv, max_len, D]; cache rows at or past each length hold NaN."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(len(lens), H * D, generator=g).to(torch.bfloat16)
    kc = torch.randn(len(lens), Hkv, max_len, D, generator=g).to(torch.bfloat16)
    for b, L in enumerate(lens):
        kc[b, :, L:] = float("nan")
    return q, kc


def count_probe(lens, H, Hkv, D, max_len=MAX_LEN, seed=SEED):
    """All keys of a (sequence, K/V head) equal: every score has the same bits, probs = 1 / n and mass_g = n_g / n."""
    g = torch.Generator().manual_seed(seed + 1)
    q = torch.randn(len(lens), H * D, generator=g).to(torch.bfloat16)
    row = torch.randn(len(lens), Hkv, 1, D, generator=g).to(torch.bfloat16)
    kc = row.expand(-1, -1, max_len, -1).clone()
    for b, L in enumerate(lens):
        kc[b, :, L:] = float("nan")
    return q, kc


def peak_targets(seg_row, L, n_seg):
    """Key 0, the last key, and the first and the last key of a segment in the middle of the row."""
    s = seg_row[:L].tolist()
    firsts = [j for j in range(L) if s[j] < n_seg and (j == 0 or s[j - 1] != s[j])]
    lasts = [j for j in range(L) if s[j] < n_seg and (j == L - 1 or s[j + 1] != s[j])]
    return [0, L - 1, firsts[len(firsts) // 2], lasts[len(lasts) // 2]]


def peak_probe(lens, H, Hkv, D, seg, n_seg, max_len=MAX_LEN, seed=SEED):
    """K rows are pseudo-random +-1 patterns, head h's query is 8 x the pattern of its target key (target kind h mod 4 of
    ``peak_targets``), scale = D^-0.5: the target scores 8 sqrt(D), every other key (8 / sqrt(D)) x a sum of D random signs.
    Returns (q, kc, tgt [B, H])."""
    g = torch.Generator().manual_seed(seed + 2)
    kc = (torch.randint(0, 2, (len(lens), Hkv, max_len, D), generator=g) * 2 - 1).float()
    q = torch.zeros(len(lens), H, D)
    tgt = torch.zeros(len(lens), H, dtype=torch.long)
    G = H // Hkv
    for b, L in enumerate(lens):
        t = peak_targets(seg[b], L, n_seg)
        for h in range(H):
            tgt[b, h] = t[h % 4]
            q[b, h] = 8 * kc[b, h // G, t[h % 4]]
        kc[b, :, L:] = float("nan")
    return q.reshape(len(lens), H * D).to(torch.bfloat16), kc.to(torch.bfloat16), tgt


# ------------------------------------------------------------------------------------------------------------------
# the reference and its mutants
# ------------------------------------------------------------------------------------------------------------------
@dataclass
class Ref:
    probs: torch.Tensor      # f64 [B, H, max_len], 0 at and past each length
    mass: torch.Tensor       # f64 [B, H, n_seg]
    S: torch.Tensor          # f64 [B, H]
    n: torch.Tensor          # f64 [B]
    n_g: torch.Tensor        # f64 [B, n_seg]
    live: torch.Tensor       # bool [B, max_len]: j < lens[b]


def reference(q, kc, lens, seg, n_seg, H, Hkv, D, scale, mutate=None) -> Ref:
    """float64, on the bf16 values given.  ``mutate``: one of MUTANTS — drop_key (key len // 2 of every row of >= 2 keys is not
    seen), dup_last (the last key counts twice), lens_minus1 (rows of >= 2 keys lose their last key), move_boundary (the first key
    of each row's second run joins the run before it), ignored_into_0 (every ignored id inside the length counts into segment 0)."""
    assert mutate is None or mutate in MUTANTS
    Bn, max_len, G = len(lens), kc.shape[2], H // Hkv
    probs = torch.zeros(Bn, H, max_len, dtype=torch.float64)
    mass = torch.zeros(Bn, H, n_seg, dtype=torch.float64)
    S, n, n_g = torch.zeros(Bn, H, dtype=torch.float64), torch.zeros(Bn, dtype=torch.float64), torch.zeros(Bn, n_seg, dtype=torch.float64)
    live = torch.zeros(Bn, max_len, dtype=torch.bool)
    for b, L in enumerate(lens):
        L = int(L)
        live[b, :L] = True
        if mutate == "lens_minus1" and L >= 2:
            L -= 1
        k = kc[b, :, :L].double().repeat_interleave(G, 0)                       # [H, L, D]
        qh = q[b].reshape(H, D).double()
        s = scale * torch.einsum("hd,hjd->hj", qh, k)
        S[b] = (scale * torch.einsum("hd,hjd->hj", qh.abs(), k.abs())).amax(-1)
        e = torch.exp(s - s.amax(-1, keepdim=True))
        if mutate == "drop_key" and L >= 2:
            e[:, L // 2] = 0.0
        if mutate == "dup_last":
            e[:, L - 1] *= 2.0
        p = e / e.sum(-1, keepdim=True)
        ids = seg[b, :L].long().clone()
        if mutate == "move_boundary":
            for j in range(1, L):
                if ids[j] != ids[j - 1] and ids[j] < n_seg and ids[j - 1] < n_seg:
                    ids[j] = ids[j - 1]
                    break
        if mutate == "ignored_into_0":
            ids[ids >= n_seg] = 0
        probs[b, :, :L] = p
        n[b] = L
        for g in range(n_seg):
            sel = ids == g
            n_g[b, g] = int(sel.sum())
            mass[b, :, g] = p[:, sel].sum(-1)
    return Ref(probs, mass, S, n, n_g, live)


def emulate_f32(q, kc, lens, seg, n_seg, H, Hkv, D, scale):
    """The definition in numpy float32, the segment sums sequential in key order.  Returns (mass f32 [B, H, n_seg], probs f32
    [B, H, max_len] with NaN at and past each length: the kernel leaves those untouched)."""
    Bn, max_len, G = len(lens), kc.shape[2], H // Hkv
    mass = np.zeros((Bn, H, n_seg), dtype=np.float32)
    probs = np.full((Bn, H, max_len), np.nan, dtype=np.float32)
    for b, L in enumerate(lens):
        k = kc[b, :, :L].float().numpy()
        qh = q[b].reshape(H, D).float().numpy()
        ids = seg[b, :L].numpy()
        for h in range(H):
            s = np.float32(scale) * (k[h // G] @ qh[h]).astype(np.float32)
            e = np.exp(s - s.max()).astype(np.float32)
            p = (e / e.sum(dtype=np.float32)).astype(np.float32)
            probs[b, h, :L] = p
            for g in range(n_seg):
                sel = p[ids == g]
                mass[b, h, g] = np.cumsum(sel, dtype=np.float32)[-1] if sel.size else np.float32(0)
    return torch.from_numpy(mass), torch.from_numpy(probs)


# ------------------------------------------------------------------------------------------------------------------
# the bound
# ------------------------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return torch.where(torch.isfinite(err), r, torch.full_like(r, float("inf")))


def mass_ratio(got_mass, R: Ref, D):
    """err / bound per element of mass, [B, H, n_seg] (inf for a non-finite value or any error where the bound is 0)."""
    rel = C1 * D * U * R.S[:, :, None] + C2 * (R.n[:, None, None] + R.n_g[:, None, :] + 8) * U
    bound = R.mass * rel + R.n_g[:, None, :] * TINY
    return _ratio((got_mass.double() - R.mass).abs(), bound)


def probs_ratio(got_probs, R: Ref, D):
    """err / bound per live element of probs (elements at or past the length read 0: they are not the kernel's)."""
    rel = C1 * D * U * R.S + C2 * (R.n[:, None] + 8) * U
    bound = R.probs * rel[:, :, None] + TINY
    live = R.live[:, None, :].expand_as(R.probs)
    err = torch.where(live, (got_probs.double() - R.probs).abs(), torch.zeros_like(R.probs))
    return _ratio(err, bound)


def worst(got_mass, got_probs, R: Ref, D):
    """(largest err / bound of mass, of probs)."""
    return float(mass_ratio(got_mass, R, D).max()), float(probs_ratio(got_probs, R, D).max())


def describe(ratio):
    idx = torch.nonzero(ratio > 1)
    return "none" if idx.numel() == 0 else f"{idx.shape[0]} elements; first at (row, head, index) {tuple(int(x) for x in idx[0])}"

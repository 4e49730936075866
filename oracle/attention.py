"""A float64 reference of softmax attention, probe inputs for which a one-key mistake is far above rounding, deliberately
wrong references (mutants) and the assertion helpers shared by tests/test_gpu_attention_exact.py (kernel output) and
tests/test_attention_probes.py (mutant output in place of a kernel's).  Plain torch: runs on the CPU or on the device.

Every reference works on "groups": q [G, H, Nq, D], k / v [G, H, Nk, D], visible [G, 1|H, Nq, Nk].  The wrappers
(prefill_ref, decode_ref, qformer_ref) turn a kernel's own layout into groups, one packed sequence / cache row / window at a
time, and return a ``Ref`` whose rows are the kernel's output rows.

Probes (all values exact in bf16; K rows of the count and bias probes are never weighed because q = 0):
  count  q = 0, V row j = one-hot e[(j + 7 h) mod P], P = 61 (D = 64) / 127 (D = 128), prime: o[d] = count_d / n exactly up to
         the final division.  One key too many or too few moves a column by >= 1 / ceil(n / P) of its value.
  peak   K row j = a pseudo-random +-1 pattern, query i = 8 x the pattern of its target t(i), scale = D^-0.5: the target's score is
         8 sqrt(D), every other score is (8 / sqrt(D)) x a sum of D random signs (sigma = 8).  |V| in [1, 2).  Output = V row t(i).
  bias   q = k = 0, table(rel) = -30 |rel - 3|, gate in [0.5, 2.5]: query i returns V row i + 3 where that key is visible (causal: V
         row i, the nearest visible key to i + 3, where key i is visible).
Exact rows are asserted with torch.equal AFTER the float64 reference has shown (never the kernel) that the target's weight is
>= 1 - 2^-12 and every |v| is <= 2 |v_t|: then |o - v_t| <= 2^-12 * 3 |v_t| < 2^-9 <= half the spacing of bf16 below |v_t| >= 1.
"""
from __future__ import annotations

from dataclasses import dataclass, fields

import torch

U = 2.0 ** -24            # f32 unit roundoff
C1 = 4                    # two f32 dot-product scores (C_DOT = 2 each) entering a weight ratio, first order
C2 = 2                    # C_DOT of the f32 accumulation over n keys; + 8 covers exp (1 ulp), the division and the rescales
W_EXACT = 1.0 - 2.0 ** -12
R_P = {"prefill64": 2.0 ** -9, "prefill128": 2.0 ** -16, "decode": 0.0, "qformer": 0.0}   # the kernel's own rounding of P

MUTANTS = ("drop_last", "admit_next", "kvlen_plus1", "dup_last", "shift_v", "swap_tiles", "rel_flip", "no_clamp")
PREFILL_LENS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 0, 129, 191, 192, 193, 255, 256, 257, 320, 385)   # one empty, in the middle
DECODE_LENS = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 319, 320)
KV_EDGES = (1, 63, 64, 65, None)       # kv_lens at the tile edges, None = the sequence's length
SEED = 1117                            # fixed by tests/test_attention_probes.py: every exact-row condition holds for it
PRIME = {64: 61, 128: 127}


def cu_of(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


def kv_lens_of(lens):
    """kv_len at the tile edges 1, 63, 64, 65 and len, cycling over the sequences (never above the length, at least 1)."""
    return [max(1, n if KV_EDGES[s % 5] is None else min(KV_EDGES[s % 5], n)) for s, n in enumerate(lens)]


def ulp_bf16(x):
    """Spacing of bf16 at |x| (float64 tensor); the subnormal spacing below 2^-126."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


# ------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------
def attention_ref(q, k, v, visible, scale, bias=None, mult=None):
    """float64 softmax attention per query and output element.  Returns (ref = sum_j p_j v_j, A = sum_j p_j |v_j|, p,
    S = max_j (scale * sum_i |q_i| |k_ji| + |bias_ij|) over the visible keys).  ``mult`` (mutants only) counts a key several
    times.  A query without a visible key has p = 0 and ref = 0."""
    q, k, v = q.double(), k.double(), v.double()
    s = scale * (q @ k.transpose(-1, -2))
    mag = scale * (q.abs() @ k.abs().transpose(-1, -2))
    if bias is not None:
        s = s + bias.double()
        mag = mag + bias.double().abs()
    vis = visible.expand(s.shape)
    s = s.masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    if mult is not None:
        e = e * mult
    den = e.sum(-1, keepdim=True)
    p = e / den.clamp_min(1e-300)
    S = mag.masked_fill(~vis, 0.0).amax(-1)
    return p @ v, p @ v.abs(), p, S


@dataclass
class Ref:
    """Per output row r (and head h): ref / A / vt [R, H, D]; S / n / pmax [R, H]; tgt [R, H] the heaviest key's index; vdom [R, H]
    every |v| of the group <= 2 |v_tgt|; seq / pos [R] the sequence (or cache row, window) and the query's position in it."""
    ref: torch.Tensor
    A: torch.Tensor
    vt: torch.Tensor
    S: torch.Tensor
    n: torch.Tensor
    pmax: torch.Tensor
    tgt: torch.Tensor
    vdom: torch.Tensor
    seq: torch.Tensor
    pos: torch.Tensor

    @staticmethod
    def cat(parts):
        return Ref(*[torch.cat([getattr(p, f.name) for p in parts]) for f in fields(Ref)])

    def rows(self, idx):
        return Ref(*[getattr(self, f.name)[idx] for f in fields(Ref)])


def _group_ref(q, k, v, visible, scale, bias, mult, vmap, seq, pos):
    """q [H, Nq, D], k / v [H, Nk, D], visible / mult [Nq, Nk] -> Ref with Nq rows."""
    if vmap is not None:
        v = v[:, vmap]
    ref, A, p, S = attention_ref(q, k, v, visible[None], scale, bias, None if mult is None else mult[None])
    pmax, tgt = p.max(-1)                                                   # [H, Nq]
    vt = torch.gather(v.double(), 1, tgt[..., None].expand(-1, -1, v.shape[-1]))
    vdom = (v.double().abs().amax(1, keepdim=True) <= 2 * vt.abs()).all(-1)
    n = visible.sum(-1)[None].expand(q.shape[0], -1)
    dev = q.device
    t = lambda x: x.transpose(0, 1).contiguous()
    return Ref(t(ref), t(A), t(vt), t(S), t(n), t(pmax), t(tgt), t(vdom),
               torch.full((q.shape[1],), seq, dtype=torch.long, device=dev), torch.as_tensor(pos, device=dev).long())


def _mutate(mutate, visible, causal, kvl, L):
    """The structural mutants on one group: returns (visible, mult, vmap).  visible [Nq, L] is modified in place."""
    mult = vmap = None
    dev = visible.device
    j = torch.arange(L, device=dev)
    if mutate in ("drop_last", "dup_last"):
        has = visible.any(-1)
        last = (visible * (j + 1)[None]).amax(-1) - 1                       # last visible key of each query
        r = torch.nonzero(has)[:, 0]
        if mutate == "drop_last":
            visible[r, last[r]] = False
        else:
            mult = torch.ones(visible.shape, dtype=torch.float64, device=dev)
            mult[r, last[r]] = 2.0
    elif mutate == "shift_v":
        vmap = (j + 1).clamp_max(L - 1)
    elif mutate == "swap_tiles":
        vmap = j.clone()
        lo = j[(j < 64) & (j + 64 < L)]
        vmap[lo], vmap[lo + 64] = lo + 64, lo
    return visible, mult, vmap


def prefill_ref(q, k, v, lens, H, D, scale, *, causal=False, kv_lens=None, rel_bias=None, rel_gate=None, rel_span=0,
                mutate=None) -> Ref:
    """icl_attn_fwd_bf16 on packed rows: q / k / v [total, H * D], sequence s owns rows cu[s] .. cu[s + 1] - 1."""
    assert mutate is None or mutate in MUTANTS
    cu, parts, dev = cu_of(lens), [], q.device
    for s, L in enumerate(lens):
        if L == 0:
            continue
        a, b = cu[s], cu[s + 1]
        g = lambda x: x[a:b].reshape(L, H, D).transpose(0, 1)
        kvl = L if kv_lens is None else min(max(int(kv_lens[s]), 1), L)
        i, j = torch.arange(L, device=dev)[:, None], torch.arange(L, device=dev)[None, :]
        visible = (j < kvl) & ((j <= i) if causal else torch.ones_like(j <= i))
        if mutate == "admit_next" and causal:
            visible = visible | ((j == i + 1) & (j < kvl))
        if mutate == "kvlen_plus1":
            visible = visible | ((j == kvl) & ((j <= i) if causal else torch.ones_like(j <= i)))
        visible, mult, vmap = _mutate(mutate, visible.clone(), causal, kvl, L)
        bias = None
        if rel_bias is not None:
            rel = (i - j) if mutate == "rel_flip" else (j - i)
            if mutate == "no_clamp":
                idx = (rel + rel_span - 1) % (2 * rel_span - 1)
            else:
                idx = rel.clamp(-(rel_span - 1), rel_span - 1) + rel_span - 1
            bias = rel_gate[a:b].double().t()[:, :, None] * rel_bias.double()[:, idx]
        parts.append(_group_ref(g(q), g(k), g(v), visible, scale, bias, mult, vmap, s, torch.arange(L)))
    return Ref.cat(parts)


def decode_ref(q, kc, vc, lens, H, D, scale, *, mutate=None) -> Ref:
    """icl_attn_decode_bf16: q [B, H * D], caches [B, H, max_len, D], one query per sequence over rows [0, lens[b])."""
    parts = []
    for b, L in enumerate(lens):
        L = int(L)
        n = L + 1 if mutate == "kvlen_plus1" and L < kc.shape[2] else L       # only the rows a mutant may touch are sliced
        visible = (torch.arange(n, device=q.device) < L)[None]
        if mutate == "kvlen_plus1":
            visible = torch.ones_like(visible)
        visible, mult, vmap = _mutate(mutate, visible.clone(), False, L, n)
        parts.append(_group_ref(q[b].reshape(H, 1, D), kc[b, :, :n], vc[b, :, :n], visible, scale, None, mult, vmap, b, [L - 1]))
    return Ref.cat(parts)


def qformer_ref(q, kv, v_off, n_audio, wpa, win, rpa, H, scale, *, mutate=None) -> Ref:
    """icl_qformer_window_xattn: window w of audio a attends rows a * rpa + w * win .. + win - 1 of kv (K at column 0, V at v_off)."""
    D, parts = 64, []
    for w in range(n_audio * wpa):
        r0 = (w // wpa) * rpa + (w % wpa) * win
        g = lambda c: kv[r0:r0 + win, c:c + H * D].reshape(win, H, D).transpose(0, 1)
        visible = torch.ones(1, win, dtype=torch.bool, device=q.device)
        visible, mult, vmap = _mutate(mutate, visible, False, win, win)
        parts.append(_group_ref(q[w].reshape(H, 1, D), g(0), g(v_off), visible, scale, None, mult, vmap, w, [win - 1]))
    return Ref.cat(parts)


# ------------------------------------------------------------------------------------------------------------------
# assertions: each returns the failing (row, head) mask; assert_* raise, naming the first failing query and its key
# ------------------------------------------------------------------------------------------------------------------
def err_bound(got, R: Ref, D, r_P):
    """|got - ref| <= ulp_bf16(max(|ref|, |got|)) + A * (r_P + C1 * D * u * S + C2 * (n + 8) * u), per element."""
    got = got.double()
    rel = r_P + C1 * D * U * R.S + C2 * (R.n.double() + 8) * U
    return ulp_bf16(torch.maximum(R.ref.abs(), got.abs())) + R.A * rel[..., None]


def fails_bound(got, R: Ref, D, r_P):
    ratio = (got.double() - R.ref).abs() / err_bound(got, R, D, r_P)
    ratio = torch.where(torch.isfinite(got.double()), ratio, torch.full_like(ratio, float("inf")))
    return (ratio > 1).any(-1), float(ratio.max())


def fails_count(got, R: Ref):
    """Within one bf16 ulp of the float64 count_d / n (a column no key feeds must be exactly 0)."""
    err = (got.double() - R.ref).abs()
    bad = (err > ulp_bf16(R.ref)) | ((R.ref == 0) & (got.double() != 0)) | ~torch.isfinite(got.double())
    return bad.any(-1)


class ProbeConditionError(AssertionError):
    """The float64 reference itself does not meet the condition under which bit equality may be asserted."""


def fails_exact(got, R: Ref, rows=None):
    """got == V row of the target, bit for bit, on ``rows`` ([R, H] bool, default all).  The condition (weight >= 1 - 2^-12,
    |v| <= 2 |v_t|) is checked on the reference for EVERY such row first: none may fail it and be skipped."""
    rows = torch.ones_like(R.vdom) if rows is None else rows
    cond = (R.pmax >= W_EXACT) & R.vdom
    if not bool((cond | ~rows).all()):
        raise ProbeConditionError(f"exact-row condition fails on the reference: {describe(R, rows & ~cond)}")
    return (got.double() != R.vt).any(-1) & rows


def describe(R: Ref, mask):
    idx = torch.nonzero(mask)
    if idx.numel() == 0:
        return "none"
    r, h = int(idx[0, 0]), int(idx[0, 1])
    return (f"{idx.shape[0]} (row, head) pairs; first: sequence {int(R.seq[r])} position {int(R.pos[r])} head {h}, heaviest key "
            f"{int(R.tgt[r, h])} (weight {float(R.pmax[r, h]):.6g}) of {int(R.n[r, h])} visible")


def assert_bound(got, R, D, r_P, what=""):
    bad, worst = fails_bound(got, R, D, r_P)
    assert not bool(bad.any()), f"{what}: err/bound {worst:.3g} > 1 at {describe(R, bad)}"
    return worst


def assert_count(got, R, what=""):
    bad = fails_count(got, R)
    assert not bool(bad.any()), f"{what}: count probe off by more than one bf16 ulp at {describe(R, bad)}"


def assert_exact(got, R, rows=None, what=""):
    bad = fails_exact(got, R, rows)
    assert not bool(bad.any()), f"{what}: output is not the target's V row at {describe(R, bad)}"


# ------------------------------------------------------------------------------------------------------------------
# probe builders: packed q / k / v [total, H * D] bf16 on the CPU (seeded), for the sequence lengths given
# ------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _unit_v(shape, g):
    """Magnitude 1 + m / 128 in [1, 2) with a random sign: exact in bf16."""
    mant = torch.randint(0, 128, shape, generator=g).double() / 128 + 1
    return mant * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)


def random_data(lens, H, D, seed=SEED, offset=False):
    """i.i.d. bf16 normal q / k / v; ``offset``: the first 16 elements of every q row are +c and of every k row -c with
    16 c^2 D^-0.5 ~ 300, so every score sits near -300 (natural units) — softmax is shift invariant, S grows."""
    g, total = _gen(seed), sum(lens)
    q, k, v = (torch.randn(total, H, D, generator=g) for _ in range(3))
    if offset:
        c = 12.25 if D == 64 else 14.5
        q[..., :16], k[..., :16] = c, -c
    return tuple(x.reshape(total, H * D).to(torch.bfloat16) for x in (q, k, v))


def probe_count(lens, H, D, seed=SEED):
    total, P = sum(lens), PRIME[D]
    q = torch.zeros(total, H, D)
    k = torch.randn(total, H, D, generator=_gen(seed))
    v = torch.zeros(total, H, D)
    for a, L in zip(cu_of(lens), lens):
        j, h = torch.arange(L)[:, None], torch.arange(H)[None, :]
        v[a:a + L].scatter_(2, ((j + 7 * h) % P)[..., None], 1.0)
    return tuple(x.reshape(total, H * D).to(torch.bfloat16) for x in (q, k, v))


def probe_peak(lens, H, D, seed=SEED, *, causal=False, kv_lens=None, head_offset=0):
    """Head h uses target map (h + head_offset) mod 5: 0 t = i, 1 t = 0, 2 t = last visible key, 3 t = first key of i's 64-key
    tile, 4 t = pseudo-random among the visible keys; every target is clamped to the last visible key."""
    g, total = _gen(seed), sum(lens)
    k = (torch.randint(0, 2, (total, H, D), generator=g) * 2 - 1).float()
    v = _unit_v((total, H, D), g).float()
    q = torch.zeros(total, H, D)
    for s, (a, L) in enumerate(zip(cu_of(lens), lens)):
        if L == 0:
            continue
        kvl = L if kv_lens is None else min(max(int(kv_lens[s]), 1), L)
        i = torch.arange(L)
        last = torch.minimum(i, torch.tensor(kvl - 1)) if causal else torch.full((L,), kvl - 1)
        u = torch.rand(L, H, generator=g)
        for h in range(H):
            t = [i, torch.zeros_like(i), last, (i // 64) * 64, (u[:, h] * (last + 1)).long()][(h + head_offset) % 5]
            q[a:a + L, h] = 8 * k[a + torch.minimum(t, last), h]
    return tuple(x.reshape(total, H * D).to(torch.bfloat16) for x in (q, k, v))


def probe_bias(lens, H, D, rel_span, seed=SEED):
    """q = k = 0; returns (q, k, v, rel_bias f32 [H, 2 * rel_span - 1], rel_gate f32 [total, H])."""
    g, total = _gen(seed), sum(lens)
    z = torch.zeros(total, H * D, dtype=torch.bfloat16)
    v = _unit_v((total, H * D), g).to(torch.bfloat16)
    rel = torch.arange(-(rel_span - 1), rel_span).float()
    table = (-30.0 * (rel - 3).abs())[None].repeat(H, 1).contiguous()
    gate = torch.rand(total, H, generator=g) * 2 + 0.5
    return z, z.clone(), v, table, gate


def bias_exact_rows(lens, H, causal, kv_lens):
    """[R, H] mask of the bias probe's exact rows (R counts the rows of the non-empty sequences, packed order) and the number
    of remaining rows the mask predicts: non-causal, query i is exact iff key i + 3 is visible (i + 3 < kv_len); causal, key i + 3
    never is, the nearest visible key is i itself and the row is exact iff i < kv_len."""
    rows, rest = [], 0
    for s, L in enumerate(lens):
        kvl = L if kv_lens is None else min(max(int(kv_lens[s]), 1), L)
        i = torch.arange(L)
        rows.append(i < kvl if causal else i + 3 < kvl)
        rest += L - (kvl if causal else max(kvl - 3, 0))
    return torch.cat(rows)[:, None].expand(-1, H), rest


# ------------------------------------------------------------------------------------------------------------------
# layouts: the packed probes as a decode cache or as Q-Former windows
# ------------------------------------------------------------------------------------------------------------------
def to_cache(k, v, lens, H, D, max_len, fill=float("nan")):
    """Packed k / v -> caches [n_seqs, H, max_len, D]; rows past each length hold ``fill``."""
    kc = torch.full((len(lens), H, max_len, D), fill, dtype=k.dtype, device=k.device)
    vc = torch.full_like(kc, fill)
    for s, (a, L) in enumerate(zip(cu_of(lens), lens)):
        kc[s, :, :L] = k[a:a + L].view(L, H, D).transpose(0, 1)
        vc[s, :, :L] = v[a:a + L].view(L, H, D).transpose(0, 1)
    return kc, vc


def last_rows(x, lens):
    """The packed row of each sequence's last position (the decode query)."""
    return x[torch.tensor(cu_of(lens)[1:]) - 1]


def to_windows(k, v, n_audio, wpa, win, rpa, H, pad=64):
    """Packed k / v of n_audio * wpa windows of ``win`` keys -> the kv buffer [n_audio * rpa, 2 * H * 64 + pad]: K at column 0, ``pad``
    unused columns, V at column v_off = H * 64 + pad; the rows no window covers hold NaN.  Returns (kv, v_off)."""
    hd = H * 64
    v_off = hd + pad
    kv = torch.full((n_audio * rpa, v_off + hd), float("nan"), dtype=k.dtype, device=k.device)
    for w in range(n_audio * wpa):
        r0 = (w // wpa) * rpa + (w % wpa) * win
        kv[r0:r0 + win, :hd] = k[w * win:(w + 1) * win]
        kv[r0:r0 + win, hd:v_off] = 0
        kv[r0:r0 + win, v_off:] = v[w * win:(w + 1) * win]
    return kv, v_off

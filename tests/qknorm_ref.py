"""References for the QK-norm decoder (Qwen3) tests: test_qknorm.py on the CPU, test_gpu_qknorm.py on the GPU.  Not a test module.

QKNormOracle      LlamaOracle with the per-head q / k RMSNorm of Qwen3Attention between the projection and RoPE.
qknorm_ref_bound  the float64 reference of the norm stage of icl_qknorm_rope_kv_bf16 and the bound of the kernel's f32 value.
kernel_case       the inputs both test modules run the kernel (or its f32 emulation) on.
qknorm_f32 / rope_f32 / emulate   a torch f32 emulation of the kernel in its own operation order (csrc/rope_kv.hip)."""
from typing import Optional

import torch

import fp64_bounds as fb
from oracle import models as om

BF16, F32 = torch.bfloat16, torch.float32
EPS = 1e-6


class QKNormOracle(om.LlamaOracle):
    """LlamaOracle whose attention normalises every q head and every k head over head_dim (gains
    ``self_attn.{q,k}_norm.weight`` [head_dim], eps = rms_eps) before the rotation, as transformers' Qwen3Attention does.  The
    ``rnd`` hook sits before the norm (the bf16 QKV buffer the kernel reads) and after it (the bf16 rounding point of
    icl_qknorm_rope_kv_bf16 between the norm and RoPE); everything else is inherited."""

    def _head_norm(self, x, name):     # x [B, T, heads, D]
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.eps) * self.sd[name].float()

    def forward_hidden(self, h, pos, cache: Optional[list] = None, attn_mask=None):
        rnd = self.rnd
        B, T, C = h.shape
        for i in range(self.n_layers):
            lp = f"model.layers.{i}."
            xn = self._rms(h, lp + "input_layernorm.weight")
            q = self._proj(xn, lp + "self_attn.q_proj").view(B, T, self.H, self.D)
            k = self._proj(xn, lp + "self_attn.k_proj").view(B, T, self.Hkv, self.D)
            v = rnd(self._proj(xn, lp + "self_attn.v_proj")).view(B, T, self.Hkv, self.D)
            q = rnd(self._head_norm(rnd(q), lp + "self_attn.q_norm.weight"))
            k = rnd(self._head_norm(rnd(k), lp + "self_attn.k_norm.weight"))
            q, k = rnd(self._rope(q, pos)), rnd(self._rope(k, pos))
            if cache is not None:
                if len(cache) <= i:
                    cache.append((k, v))
                else:
                    cache[i] = (torch.cat([cache[i][0], k], 1), torch.cat([cache[i][1], v], 1))
                k, v = cache[i]
            Tk = k.shape[1]
            if self.Hkv != self.H:
                rep = self.H // self.Hkv
                k, v = k.repeat_interleave(rep, dim=2), v.repeat_interleave(rep, dim=2)
            mask = (torch.arange(Tk)[None, :] > (torch.arange(T)[:, None] + (Tk - T)))[None, None]      # causal
            if attn_mask is not None:
                mask = mask | ~attn_mask[:, None, None, :].bool()
            a = rnd(om._mha(q.reshape(B, T, C), k.reshape(B, Tk, C), v.reshape(B, Tk, C), self.H, self.D ** -0.5, mask=mask))
            h = h + self._proj(a, lp + "self_attn.o_proj")
            xn = self._rms(h, lp + "post_attention_layernorm.weight")
            g = om._lin(xn, self.sd, lp + "mlp.gate_proj", rnd)
            u = om._lin(xn, self.sd, lp + "mlp.up_proj", rnd)
            h = h + om._lin(rnd(torch.nn.functional.silu(g) * u), self.sd, lp + "mlp.down_proj", rnd)
        return h


def qknorm_ref_bound(x, gamma, eps):
    """(ref, e) of n = x rsqrt(mean(x^2) + eps) gamma over the last axis (length D = 64 or 128) as an f32 value, per element in
    float64.  x bf16 and gamma f32 are taken as data, eps is the f32 the C ABI passes.  With u = 2^-24 and the kernel's order
    (csrc/rope_kv.hip):

      * a bf16 square is exact in f32 (16 significant bits), so the sum of squares errs only in its additions.  A lane adds its
        eight squares in series (the first addition, to 0, is exact: 7 roundings); the D / 8 lane sums are folded by an xor
        butterfly of L = log2(D / 8) levels.  Every term is >= 0, so each addition a term passes through costs it at most u
        relative:  |ss^ - ss| <= A u ss,  A = 7 + L  (11 at D = 128, 10 at D = 64).
      * ss (1 / D) is a scaling by a power of two: exact.
      * t^ = fl(m^ + eps):  |t^ - t| <= A u m + u t <= (A + 1) u t,  as m <= t.
      * r^ = rsqrtf(t^): the argument's error moves r by half of it, (A + 1) u / 2 relative; rsqrtf is documented at 1 ulp
        (2^-23 = 2u relative), taken at twice that: 4u.
      * (x r^) gamma: two products, 2u.

    e = ((A + 1) / 2 + 6) u |ref|  —  12 u |ref| at D = 128, 11.5 u |ref| at D = 64 — times (1 + 2^-16) for the second-order
    terms (of order (12 u)^2) and for squares below the smallest normal (|x| < 2^-63: an absolute 2^-149 each, against eps).
    The domain |x| <= 2^60 keeps ss <= 128 * 2^120 finite.  The kernel's bf16 output is judged by
    fb.bf16_interval(ref - e, ref + e)."""
    D = x.shape[-1]
    assert D in (64, 128)
    A = 7 + {64: 3, 128: 4}[D]
    x64, g64 = x.double(), gamma.double()
    t = x64.pow(2).mean(-1, keepdim=True) + fb.f32_scalar(eps)
    ref = x64 * torch.rsqrt(t) * g64
    return ref, ((A + 1) / 2.0 + 6.0) * fb.U * ref.abs() * (1.0 + 2.0 ** -16)


# ---- the kernel test's inputs ---------------------------------------------------------------------------------------------------
KINDS = ("normal", "small", "large", "zero", "spike")


def kernel_case(M, H, Hkv, D, seed=0):
    """q [M, H, D], k, v [M, Hkv, D] bf16 and q_gamma, k_gamma f32 [D].  Head row j of qkv row m (q heads, then k, then v) is of
    kind KINDS[(m + j) % 5]: normal; scaled by 2^-20 (eps dominates); scaled by 2^20; all zero; one element of 2^8 among
    elements of 2^-10 N(0, 1); a v row is never all zero (a normed v must show).  The gains are 1 + 0.3 N(0, 1), drawn apart for q and k."""
    g = torch.Generator().manual_seed(1000 * seed + 97 * H + 13 * Hkv + D + M)
    n = H + 2 * Hkv
    x = torch.randn(M, n, D, generator=g)
    for m in range(M):
        for j in range(n):
            kind = KINDS[(m + j) % 5] if j < H + Hkv else ("normal", "small", "large", "spike")[(m + j) % 4]
            if kind == "small":
                x[m, j] *= 2.0 ** -20
            elif kind == "large":
                x[m, j] *= 2.0 ** 20
            elif kind == "zero":
                x[m, j] = 0.0
            elif kind == "spike":
                x[m, j] *= 2.0 ** -10
                x[m, j, int(torch.randint(0, D, (1,), generator=g))] = 256.0
    x = x.to(BF16)
    gq = (1.0 + 0.3 * torch.randn(D, generator=g)).float()
    gk = (1.0 + 0.3 * torch.randn(D, generator=g)).float()
    return x[:, :H].contiguous(), x[:, H:H + Hkv].contiguous(), x[:, H + Hkv:].contiguous(), gq, gk


def rope_tables(D, max_len):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=F32) / D))
    ang = torch.arange(max_len, dtype=F32)[:, None] * inv[None]
    return ang.cos(), ang.sin()


# ---- f32 emulation of the kernel, in its order ------------------------------------------------------------------------------------
def qknorm_f32(x, gamma, eps, *, use_eps=True, mean_over=None, gamma_by_chunk=False, round_bf16=True):
    """The norm stage of rope_kv_rows_kernel on x [..., D] bf16 in f32: a lane's eight squares added in element order, the
    xor butterfly over the D / 8 lanes, rsqrt(ss / D + eps), (x r) gamma, one bf16 rounding.  The keyword arguments are the
    one-mistake variants of test_qknorm.py."""
    D = x.shape[-1]
    xf = x.float()
    sq = (xf * xf).view(*xf.shape[:-1], D // 8, 8)
    s = torch.zeros_like(sq[..., 0])
    for j in range(8):
        s = s + sq[..., j]
    lanes = torch.arange(D // 8)
    o = 1
    while o < D // 8:
        s = s + s[..., lanes ^ o]
        o <<= 1
    t = s[..., :1] / float(mean_over or D)                # every lane holds the same sum; a power of two: exact
    if use_eps:
        t = t + torch.tensor(eps, dtype=F32)
    r = torch.rsqrt(t)
    g = gamma.float()
    if gamma_by_chunk:                      # the lane's chunk index where the element's belongs
        g = g[torch.arange(D) // 8]
    n = (xf * r) * g
    return n.to(BF16) if round_bf16 else n


def rope_f32(x, c, s):
    """rope_rot8 on x [M, heads, D] (bf16 or unrounded f32) at cos / sin [M, 1, D / 2]: products and sums rounded separately in
    f32, one bf16 rounding."""
    xf = x.float()
    h = xf.shape[-1] // 2
    a, b = xf[..., :h], xf[..., h:]
    return torch.cat([a * c - b * s, b * c + a * s], -1).to(BF16)


def emulate(q, k, v, gq, gk, eps, cos, sin, pos, mutant=None):
    """(q', k', v') of the launch, v' being what reaches the cache, from the f32 emulation; ``mutant`` names one deliberate
    mistake: no_eps, mean_2d, mean_half, k_with_q_gamma, gamma_by_chunk, norm_after_rope, no_bf16_round, v_normed."""
    c, s = cos[pos][:, None], sin[pos][:, None]
    kw = {"no_eps": dict(use_eps=False), "mean_2d": dict(mean_over=2 * q.shape[-1]), "mean_half": dict(mean_over=q.shape[-1] // 2),
          "gamma_by_chunk": dict(gamma_by_chunk=True), "no_bf16_round": dict(round_bf16=False)}.get(mutant, {})
    gk_used = gq if mutant == "k_with_q_gamma" else gk
    if mutant == "norm_after_rope":
        qo, ko = qknorm_f32(rope_f32(q, c, s), gq, eps), qknorm_f32(rope_f32(k, c, s), gk, eps)
    else:
        qo, ko = rope_f32(qknorm_f32(q, gq, eps, **kw), c, s), rope_f32(qknorm_f32(k, gk_used, eps, **kw), c, s)
    vo = qknorm_f32(v, gk, eps) if mutant == "v_normed" else v.clone()
    return qo, ko, vo


def same_values(a, b):
    """Bit equality of two bf16 tensors with +0 = -0 (NaN equals the NaN of the same bits)."""
    za, zb = torch.where(a == 0, torch.zeros_like(a), a), torch.where(b == 0, torch.zeros_like(b), b)
    return torch.equal(za.contiguous().view(torch.int16), zb.contiguous().view(torch.int16))


def norm_check(out, x, gamma, eps):
    """(mask of the elements of ``out`` outside the norm's interval, err / bound figure)."""
    ref, e = qknorm_ref_bound(x, gamma, eps)
    lo, hi = fb.bf16_interval(ref, e)
    return ~fb.in_interval(out, lo, hi), fb.interval_ratio(out, ref, lo, hi)

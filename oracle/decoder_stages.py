"""ORACLE (test infrastructure only — never imported by the product path).

Float64 specifications of the single stages of the LLM decoder chain (LlamaHIP.prefill / _last_layer_rows / decode_step /
logits of runtime/engines.py), written from the model definition (oracle/models.py: ``LlamaOracle``; tests/qknorm_ref.py:
``QKNormOracle``) — not from runtime/engines.py.  A stage is a plain function over LOGICAL tensors (a layer's rows, a head's
keys), taking its weights from the state dict (rounded to bf16 where the oracle's ``rnd`` rounds them) and its input from
whoever calls it: the stage check of tests/decoder_stage_check.py passes the logical contents of the previous stage's ACTUAL
output (teacher forcing), so errors do not add up over the chain and the per-kernel bounds of tests/fp64_bounds.py,
tests/qknorm_ref.py and oracle/attention.py apply unchanged.  Each stage returns ``(ref, bound)`` (the bound is for the kernel's
f32 value; the store to bf16 is the judge's business), ``(dot, mag)`` where the caller chooses between two kernel families'
bounds, or an ``oracle.attention.Ref``.  No stage looks at a launch's strides, offsets, counts, ``pos`` / ``sid`` tensors or
the cache's geometry: a reference built from those would agree with a wrong one.

``check_packed_llama`` asserts that the re-laid-out operands of runtime/packing.py (and the FP8 weight mode's copies) a stage
depends on are bit-equal to the state dict's, re-laid-out here from the definition.
"""
from __future__ import annotations

import torch

import fp64_bounds as fb                      # tests/fp64_bounds.py
import fp8_ref                                # tests/fp8_ref.py: the FP8 row-quantisation contract
import qknorm_ref as qr                       # tests/qknorm_ref.py: the bound of the per-head q / k RMSNorm

from . import attention as oa
from .encoder_stages import _p, _w, rnd64, same_bits

BF16, F32 = torch.bfloat16, torch.float32
LORA_PAD = 64                                 # the augmentation columns of the packed QKV projection (runtime/packing.py)
PROJ = ("q_proj", "k_proj", "v_proj")


def layer_prefix(prefix, i):
    return f"{prefix}model.layers.{i}."


def proj_rows(cfg):
    """(first row, rows) of q, k and v in the fused projection's output: q takes n_heads head_dim, k and v kv_heads head_dim."""
    q, kv = cfg.n_heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim
    return dict(q_proj=(0, q), k_proj=(q, kv), v_proj=(q + kv, kv))


def k_aug(cfg):
    return cfg.hidden + (LORA_PAD if cfg.lora_rank else 0)


# ---------------------------------------------------------------------------------------------------------------------------
# the stages
# ---------------------------------------------------------------------------------------------------------------------------
def embed(sd, prefix, src, speech, dev):
    """Row r is the bf16 embedding of token ``src[r]`` (>= 0) or speech row ``-src[r] - 1`` (f32, copied): exact, f32."""
    table = sd[prefix + "model.embed_tokens.weight"].float().to(BF16).float().to(dev)
    out = torch.empty(len(src), table.shape[1], dtype=F32, device=dev)
    for r, s in enumerate(src):
        out[r] = table[s] if s >= 0 else speech[-s - 1]
    return out


def rms_norm(sd, name, x, eps):
    """RMSNorm ``name`` of the rows of x [M, hidden] f32."""
    return fb.norm_ref_bound(x, _p(sd, name, x.device), None, eps, rms=True)


def lora_weight(sd, lp, cfg, dev):
    """The A matrices of the layer's LoRA targets, one under the other, times alpha / r, as bf16 data: the rule the packer
    documents (the scale is folded into A so that the down-projection is a plain product)."""
    a = torch.cat([sd[lp + f"self_attn.{t}.lora_A.weight"].float() for t in cfg.lora_targets], 0) * cfg.lora_scale
    return rnd64(a).to(dev)


def lora_down(sd, lp, cfg, xn):
    """xn [M, hidden] bf16 -> (dot, mag) of t = xn (s A)^T, [M, r * targets]; the caller applies the bound of the kernel that ran
    (the skinny GEMM: gemm_ref_bound at K = hidden; icl_lora_down_bf16: lora_ref_bound, which this is with scale 1)."""
    return fb.dot64(xn, lora_weight(sd, lp, cfg, xn.device))


def qkv_weight(sd, lp, cfg, dev):
    """[q; k; v] rows over the columns [x | t]: projection ``n`` sees W_n x + B_n t_n (its own rank block of t, if it is a
    LoRA target), float64 of the bf16 weights; the bias (or None)."""
    r, nt = cfg.lora_rank, len(cfg.lora_targets) if cfg.lora_rank else 0
    rows = []
    for n in PROJ:
        w = _w(sd, lp + f"self_attn.{n}.weight", dev)
        ext = torch.zeros(w.shape[0], nt * r, dtype=torch.float64, device=dev)
        if r and n in cfg.lora_targets:
            ti = cfg.lora_targets.index(n)
            ext[:, ti * r:(ti + 1) * r] = _w(sd, lp + f"self_attn.{n}.lora_B.weight", dev)
        rows.append(torch.cat([w, ext], 1))
    bias = torch.cat([_p(sd, lp + f"self_attn.{n}.bias", dev) for n in PROJ]) if cfg.qkv_bias else None
    return torch.cat(rows), bias


def qkv(sd, lp, cfg, xn, t, which=PROJ):
    """xn [M, hidden] bf16 and t [M, r * targets] bf16 (or None) -> the projections ``which`` side by side; K = k_aug(cfg), the
    depth of the kernel's accumulation over the augmented row (its zero tail adds exact zeros)."""
    w, bias = qkv_weight(sd, lp, cfg, xn.device)
    sel = torch.cat([torch.arange(r0, r0 + nr) for r0, nr in (proj_rows(cfg)[n] for n in which)]).to(xn.device)
    x = xn if t is None else torch.cat([xn, t], 1)
    dot, mag = fb.dot64(x, w[sel])
    return fb.gemm_ref_bound(dot, mag, k_aug(cfg), bias=None if bias is None else bias[sel])


def rope_tables(cfg, dev):
    """cos / sin f32 [max_pos, head_dim / 2] of HF's rotary embedding, taken in f32 as transformers takes them."""
    D = cfg.head_dim
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, D, 2, dtype=F32) / D))
    ang = torch.arange(cfg.max_pos, dtype=F32)[:, None] * inv[None, :]
    return ang.cos().to(dev), ang.sin().to(dev)


def rope(cfg, x, positions):
    """x [M, heads, D] bf16, row m at position ``positions[m]`` -> (ref, e) of the rotate-half rotation."""
    cos, sin = rope_tables(cfg, x.device)
    p = torch.as_tensor(positions, device=x.device).long()
    return fb.rope_ref_bound(x, cos[p][:, None], sin[p][:, None])


def head_norm(sd, name, cfg, x):
    """Qwen3: RMSNorm over head_dim of every head row of x [M, heads, D] bf16 with the gain ``name``."""
    return qr.qknorm_ref_bound(x, _p(sd, name, x.device), cfg.rms_eps)


def head_norm_rope(sd, name, cfg, x, positions):
    """icl_qknorm_rope_kv_bf16 leaves only the rotated row: (ref, e) of rope(bf16(norm(x))).  The norm's bf16 value n lies in
    [lo, hi] = bf16_interval of ``head_norm`` (its own bound); with m the middle and r the half width of that interval, and the
    rotation linear in n,  |rope(n) - rope(m)| <= |c| r_a + |s| r_b  per element, to which the rotation's own rounding
    (rope_ref_bound, taken at the largest magnitudes |m| + r) is added.  Where lo = hi (almost everywhere) this is rope_ref_bound."""
    ref_n, e_n = head_norm(sd, name, cfg, x)
    lo, hi = fb.bf16_interval(ref_n, e_n)
    m, r = (lo + hi) / 2, (hi - lo) / 2
    cos, sin = rope_tables(cfg, x.device)
    p = torch.as_tensor(positions, device=x.device).long()
    c, s = cos[p][:, None].double(), sin[p][:, None].double()
    ref, _ = fb.rope_ref_bound(m, c, s)
    h = x.shape[-1] // 2
    ra, rb = r[..., :h], r[..., h:]
    ma, mb = m[..., :h].abs() + ra, m[..., h:].abs() + rb
    spread = torch.cat([c.abs() * ra + s.abs() * rb, c.abs() * rb + s.abs() * ra], -1)
    mags = torch.cat([c.abs() * ma + s.abs() * mb, c.abs() * mb + s.abs() * ma], -1)
    return ref, spread + fb.U * mags + fb.U * (ref.abs() + spread)


def causal_attention(q, k, v, lens, cfg):
    """Causal softmax attention over a ragged pack: q [sum lens, H D], k / v [sum lens, Hkv D] (rotated), sequence s over its
    own rows; query head h reads K/V head h // group."""
    H, Hkv, D = cfg.n_heads, cfg.kv_heads, cfg.head_dim
    M = q.shape[0]
    rep = lambda x: x.reshape(M, Hkv, D).repeat_interleave(H // Hkv, 1).reshape(M, H * D)
    return oa.prefill_ref(q, rep(k), rep(v), list(lens), H, D, D ** -0.5, causal=True)


def cached_attention(q, keys, values, cfg):
    """One query row per sequence over the positions its cache must hold: q [B, H D]; keys[b] / values[b] [Hkv, len_b, D]
    (any float dtype: a dequantised FP8 row is float64 data)."""
    H, Hkv, D = cfg.n_heads, cfg.kv_heads, cfg.head_dim
    parts = []
    for b, (k, v) in enumerate(zip(keys, values)):
        k, v = k.repeat_interleave(H // Hkv, 0), v.repeat_interleave(H // Hkv, 0)
        n = k.shape[1]
        vis = torch.ones(1, n, dtype=torch.bool, device=q.device)
        parts.append(oa._group_ref(q[b].reshape(H, 1, D), k, v, vis, D ** -0.5, None, None, None, b, [n - 1]))
    return oa.Ref.cat(parts)


def linear(sd, name, x, *, residual=None):
    w = _w(sd, name + ".weight", x.device)
    dot, mag = fb.dot64(x, w)
    return fb.gemm_ref_bound(dot, mag, w.shape[1], residual=residual)


def gu_interleaved(g, u):
    """Gate and up rows in blocks of 16: the layout the SwiGLU epilogue reads (rows 32 j .. 32 j + 15 gate, the next 16 up)."""
    I, h = g.shape
    return torch.stack([g.view(I // 16, 16, h), u.view(I // 16, 16, h)], dim=1).reshape(2 * I, h)


def swiglu(sd, lp, xn):
    """silu(gate_proj x) * up_proj x, [M, ffn]."""
    dev = xn.device
    w = gu_interleaved(_w(sd, lp + "mlp.gate_proj.weight", dev), _w(sd, lp + "mlp.up_proj.weight", dev))
    dot, mag = fb.dot64(xn, w)
    return fb.swiglu_ref_bound(dot, mag, w.shape[1])


def fp8_row(x):
    """Rows x [..., D] bf16 -> (e4m3 bytes, f32 scale 2^e, the dequantised row as float64)."""
    q, s, _ = fp8_ref.ref_q(x)
    return q, s, dequant(q, s)


def dequant(q, s):
    return q.view(torch.float8_e4m3fn).double() * s.double()[..., None]


# ---------------------------------------------------------------------------------------------------------------------------
# the packed operands
# ---------------------------------------------------------------------------------------------------------------------------
def packed_rows(sd, lp, cfg):
    """The four GEMM weights of a layer re-laid-out from the definition, bf16, on the state dict's device: wqkv [q; k; v rows |
    each LoRA target's B in its own rank block of the augmentation columns | zero tail], wo, wgu (gate / up in blocks of 16 rows),
    wdown."""
    h, r = cfg.hidden, cfg.lora_rank
    bf = lambda key: sd[lp + key].float().to(BF16)
    want = torch.zeros(sum(nr for _, nr in proj_rows(cfg).values()), k_aug(cfg), dtype=BF16, device=sd[lp + "mlp.up_proj.weight"].device)
    for n, (r0, nr) in proj_rows(cfg).items():
        want[r0:r0 + nr, :h] = bf(f"self_attn.{n}.weight")
        if r and n in cfg.lora_targets:
            ti = cfg.lora_targets.index(n)
            want[r0:r0 + nr, h + ti * r:h + (ti + 1) * r] = bf(f"self_attn.{n}.lora_B.weight")
    return dict(wqkv=want, wo=bf("self_attn.o_proj.weight"), wgu=gu_interleaved(bf("mlp.gate_proj.weight"), bf("mlp.up_proj.weight")),
                wdown=bf("mlp.down_proj.weight"))


def w_prime_state(sd, cfg, prefix):
    """The checkpoint of the bf16 model the FP8 weight mode computes: every packed GEMM weight rounded row by row to its FP8
    value W' (tests/fp8_ref.py) and split back out under the names the definition reads.  On the state dict's device."""
    h, I, r = cfg.hidden, cfg.ffn, cfg.lora_rank
    out = dict(sd)
    for i in range(cfg.n_layers):
        lp = layer_prefix(prefix, i)
        rows = {k: fp8_ref.ref_q(v)[2].float() for k, v in packed_rows(sd, lp, cfg).items()}
        for n, (r0, nr) in proj_rows(cfg).items():
            out[lp + f"self_attn.{n}.weight"] = rows["wqkv"][r0:r0 + nr, :h]
            if r and n in cfg.lora_targets:
                ti = cfg.lora_targets.index(n)
                out[lp + f"self_attn.{n}.lora_B.weight"] = rows["wqkv"][r0:r0 + nr, h + ti * r:h + (ti + 1) * r]
        gu = rows["wgu"].view(I // 16, 2, 16, h)
        out[lp + "mlp.gate_proj.weight"], out[lp + "mlp.up_proj.weight"] = gu[:, 0].reshape(I, h), gu[:, 1].reshape(I, h)
        out[lp + "self_attn.o_proj.weight"], out[lp + "mlp.down_proj.weight"] = rows["wo"], rows["wdown"]
    return out


def check_packed_llama(sd, rt, prefix="llama_model."):
    """``rt``: a LlamaHIP.  ``sd``: the checkpoint its weights were packed from (in the FP8 weight mode: the ORIGINAL one; the
    model definition is then evaluated on ``w_prime_state(sd, cfg, prefix)``)."""
    w, cfg = rt.w, rt.w.cfg
    dev = w.embed.device
    r = cfg.lora_rank
    assert w.k_aug == k_aug(cfg)
    cos, sin = rope_tables(cfg, dev)
    assert same_bits(w.rope_cos, cos) and same_bits(w.rope_sin, sin), "packing: rope_cos / rope_sin"
    assert same_bits(w.embed, sd[prefix + "model.embed_tokens.weight"].float().to(BF16).to(dev)), "packing: embed"
    assert same_bits(w.lm_head, sd[prefix + "lm_head.weight"].float().to(BF16).to(dev)), "packing: lm_head"
    for i, L in enumerate(w.layers):
        lp = layer_prefix(prefix, i)
        rows = packed_rows(sd, lp, cfg)
        for k, (name, row) in enumerate(rows.items()):
            if rt.weight_dtype == "fp8":       # W' is the fp8 rounding of W, and the fp8 copy + scales dequantise to W' bit for bit
                q, s, wp = fp8_ref.ref_q(row)
                assert same_bits(getattr(L, name), wp.to(dev)), f"packing: layer {i} {name} is not the FP8 rounding W' of W"
                fq, fs = L.fp8[k]
                assert same_bits(fs, s.to(dev)), f"packing: layer {i} {name} fp8 scales"
                assert torch.equal(fq, fp8_ref.ref_pack(q).to(dev)), f"packing: layer {i} {name} fp8 decode-packed bytes"
                assert same_bits(dequant(q, s).to(BF16), wp), f"packing: layer {i} {name}: q * 2^e is not W'"
            else:
                assert same_bits(getattr(L, name), row.to(dev)), f"packing: layer {i} {name}"
        if r:
            a = lora_weight(sd, lp, cfg, dev)
            assert same_bits(L.lora_a, a.to(BF16)), f"packing: layer {i} lora_a is not bf16(A * alpha / r)"
            # the definition scales x A^T, the packer A: the same number where the scale is a power of two (no rounding moves)
            plain = torch.cat([rnd64(sd[lp + f"self_attn.{t}.lora_A.weight"]) for t in cfg.lora_targets], 0).to(dev)
            assert torch.equal(a, plain * cfg.lora_scale), "the LoRA scale is not exact in bf16: folding it into A moves a rounding"
        for name, key in (("rms1", "input_layernorm.weight"), ("rms2", "post_attention_layernorm.weight")):
            assert same_bits(getattr(L, name), sd[lp + key].float().to(dev)), f"packing: layer {i} {name}"
        if cfg.qkv_bias:
            assert same_bits(L.bqkv, torch.cat([sd[lp + f"self_attn.{n}.bias"].float() for n in PROJ]).to(dev)), "packing: bqkv"
        if cfg.qk_norm:
            assert same_bits(L.q_gamma, sd[lp + "self_attn.q_norm.weight"].float().to(dev)), "packing: q_gamma"
            assert same_bits(L.k_gamma, sd[lp + "self_attn.k_norm.weight"].float().to(dev)), "packing: k_gamma"
    assert same_bits(w.norm, sd[prefix + "model.norm.weight"].float().to(dev)), "packing: norm"

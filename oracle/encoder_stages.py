"""ORACLE (test infrastructure only — never imported by the product path).

Float64 specifications of the single stages of the audio encoder chains, written from the model definitions of oracle/models.py
(``whisper_encoder``, ``qwen_audio_features``, ``beats_encoder``, ``qformer``, ``salmonn_fuse_qformer``) — not from
runtime/engines.py.  A stage is a plain function over LOGICAL tensors (a clip's frames, a layer's rows), taking its weights from
the state dict (rounded to bf16 where the oracle's ``rnd`` rounds them) and its input from whoever calls it: the stage check of
tests/encoder_stage_check.py passes the logical contents of the previous stage's ACTUAL output, so errors do not add up over a
chain and the per-kernel bounds of tests/fp64_bounds.py and oracle/attention.py apply unchanged.  Each stage returns
``(ref, bound)`` (the bound is for the kernel's f32 value; the store to bf16 is the judge's business) or, for attention, an
``oracle.attention.Ref``.  No stage looks at a launch's strides, offsets or counts: a reference built from those would agree
with a wrong stride.

``check_packed_*`` assert that the re-laid-out weights of runtime/packing.py a stage depends on are bit-equal to the state
dict's, re-laid-out here from the definition: a difference is a finding in packing.py, not something a bound absorbs.

Plain torch, any device: the state dict stays on the CPU (the weight-norm of the positional conv is taken there, in f32, as
``beats_encoder`` and ``pack_beats`` take it) and each weight moves to the device of the activations when a stage needs it.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import fp64_bounds as fb                      # tests/fp64_bounds.py: the bounds every kernel family is already judged by

from . import attention as oa
from . import audio_frontend as af
from . import models as om

BF16 = torch.bfloat16


def rnd64(t):
    """The oracle's ``rnd`` (bf16_round), as float64 data."""
    return t.float().to(BF16).double()


def _w(sd, key, dev):
    return rnd64(sd[key]).to(dev)


def _p(sd, key, dev):
    """A parameter the HIP path keeps in f32 (bias, gain, table)."""
    return sd[key].float().to(dev)


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(iv), b.to(a.device).contiguous().view(iv))


def n_layers_of(sd, stem):
    """1 + the largest i of the keys ``<stem><i>.…``."""
    return 1 + max(int(k[len(stem):].split(".")[0]) for k in sd if k.startswith(stem))


# ---------------------------------------------------------------------------------------------------------------------------
# generic pieces
# ---------------------------------------------------------------------------------------------------------------------------
def conv1d64(x, w, stride, pad):
    """conv1d as its definition, in float64: x [B, T, Cin], w [Cout, Cin, k] -> (sum, sum of magnitudes) [B, T_out, Cout],
    out[b, t, o] = sum_{c, j} w[o, c, j] xpad[b, stride t + j, c] with ``pad`` zero frames on either side."""
    B, _, cin = x.shape
    k = w.shape[2]
    xp = F.pad(x.double(), (0, 0, pad, pad))
    a = xp.unfold(1, k, stride).reshape(B, -1, cin * k)                 # [B, T_out, (c, j)]
    return fb.dot64(a, w.reshape(w.shape[0], cin * k))


def linear(sd, names, x, *, residual=None, gelu=False):
    """nn.Linear ``names`` (several: their outputs side by side, a missing bias is zero) on x [M, K], [+ GELU] [+ residual]."""
    if isinstance(names, str):
        names = [names]
    dev = x.device
    w = torch.cat([_w(sd, n + ".weight", dev) for n in names])
    bias = None
    if any(n + ".bias" in sd for n in names):
        bias = torch.cat([_p(sd, n + ".bias", dev) if n + ".bias" in sd
                          else torch.zeros(sd[n + ".weight"].shape[0], device=dev) for n in names])
    dot, mag = fb.dot64(x, w)
    return fb.gemm_ref_bound(dot, mag, w.shape[1], bias=bias, residual=residual, gelu=gelu)


def layer_norm(sd, name, x, eps, *, res=None, alpha=1.0):
    """LayerNorm ``name`` of x + alpha res, rows of x [M, N]."""
    dev = x.device
    return fb.norm_ref_bound(x, _p(sd, name + ".weight", dev), _p(sd, name + ".bias", dev), eps, res=res, alpha=alpha)


def self_attention(qkv, lens, n_heads, *, kv_lens=None, rel_bias=None, rel_gate=None):
    """Softmax attention of packed rows qkv [sum lens, 3 C] (q | k | v side by side, C = n_heads D), sequence s over its own
    ``lens[s]`` rows with the first ``kv_lens[s]`` of them as keys, scale D^-0.5; ``rel_bias`` [H, 2 span - 1] (offsets
    -(span - 1) .. span - 1 of key - query) times ``rel_gate`` [rows, H] is added to the scores."""
    C = qkv.shape[1] // 3
    D = C // n_heads
    span = 0 if rel_bias is None else (rel_bias.shape[1] + 1) // 2
    return oa.prefill_ref(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], list(lens), n_heads, D, D ** -0.5, kv_lens=kv_lens,
                          rel_bias=rel_bias, rel_gate=rel_gate, rel_span=span), D


# ---------------------------------------------------------------------------------------------------------------------------
# log-mel (K1)
# ---------------------------------------------------------------------------------------------------------------------------
def logmel(wav, n_mels):
    """One clip's samples (1-D, any length) -> (ref, bound) [n_mels, 3000]."""
    return fb.whisper_ref_bound(torch.from_numpy(af.whisper_logmel(np.asarray(wav, dtype=np.float32), n_mels, as_f64=True)))


def xt_of_spec(spec, width):
    """The conv stem's operand of a spectrogram [n, n_mels, 3000]: xt[b, 1 + t, m] = bf16(spec[b, m, t]); rows 0 and 3001 and
    the columns >= n_mels are zero."""
    n, n_mels, T = spec.shape
    xt = torch.zeros(n, T + 2, width, dtype=BF16, device=spec.device)
    xt[:, 1:T + 1, :n_mels] = spec.transpose(1, 2).to(BF16)
    return xt


# ---------------------------------------------------------------------------------------------------------------------------
# Whisper encoder (K2, K3) and the Qwen2-Audio tower (K13)
# ---------------------------------------------------------------------------------------------------------------------------
MEL_PAD = 128       # the conv stem's GEMM runs over mel rows padded to 128 columns: the depth of its f32 accumulation


def check_packed_whisper(sd, w, p):
    c1 = sd[p + "conv1.weight"].float().to(BF16)                         # [d, n_mels, 3]
    d, n_mels, _ = c1.shape
    want = torch.zeros(d, 3, MEL_PAD, dtype=BF16)
    want[:, :, :n_mels] = c1.permute(0, 2, 1)                            # tap-major, mel-minor, zero past n_mels
    assert same_bits(w.conv1_w, want.reshape(d, 3 * MEL_PAD)), "packing: conv1_w is not the tap-major bf16 image of conv1.weight"
    c2 = sd[p + "conv2.weight"].float().to(BF16)                         # [d, d, 3]
    assert same_bits(w.conv2_w, c2.permute(0, 2, 1).reshape(d, 3 * d)), "packing: conv2_w is not the tap-major bf16 image of conv2.weight"


def whisper_conv1(sd, p, mel):
    """mel [n, 3000, n_mels] (the bf16 frames the stem reads) -> conv1 (k 3, pad 1) + GELU, [n, 3000, d]."""
    dev = mel.device
    dot, mag = conv1d64(mel, _w(sd, p + "conv1.weight", dev), 1, 1)
    return fb.gemm_ref_bound(dot, mag, 3 * MEL_PAD, bias=_p(sd, p + "conv1.bias", dev), gelu=True)


def whisper_conv2(sd, p, x1):
    """x1 [n, 3000, d] (conv1's output; the padding frames are zero by definition) -> conv2 (k 3, stride 2, pad 1) + GELU +
    positional embedding, [n, 1500, d]."""
    dev = x1.device
    w = _w(sd, p + "conv2.weight", dev)
    dot, mag = conv1d64(x1, w, 2, 1)
    return fb.gemm_ref_bound(dot, mag, 3 * w.shape[1], bias=_p(sd, p + "conv2.bias", dev),
                             residual=_p(sd, p + "embed_positions.weight", dev), gelu=True)


def qwen_key_lens(mel_lens):
    return [om.qwen_audio_lengths(int(m))[0] for m in mel_lens]


def pool_pairs(h):
    """h [n, T, d] -> (frames 2t, frames 2t + 1), each [n, T / 2, d]: AvgPool1d(2, 2) averages these."""
    return h[:, 0::2], h[:, 1::2]


# ---------------------------------------------------------------------------------------------------------------------------
# BEATs (K4, K5)
# ---------------------------------------------------------------------------------------------------------------------------
def _fwd_mask(feat_len, mask):              # BEATs.forward_padding_mask, as in beats_encoder
    extra = mask.size(1) % feat_len
    if extra > 0:
        mask = mask[:, :-extra]
    return mask.view(mask.size(0), feat_len, -1).all(-1)


def beats_shape(padded_len, valid_len):
    """(fbank frames, tokens T, padding mask [T] bool) of one clip processed over ``padded_len`` samples of which ``valid_len``
    are audio: forward_padding_mask applied twice (samples -> frames -> tokens)."""
    nf = af.kaldi_num_frames(int(padded_len))
    T = (nf // 16) * 8
    pad = (torch.arange(int(padded_len)) >= int(valid_len))[None]
    return nf, T, _fwd_mask(T, _fwd_mask(nf, pad))[0]


def fbank(wav, mean, std):
    """One clip's samples (1-D) -> (ref, bound) [frames, 128]; mean / std as the kernel receives them (f32)."""
    m32, s32 = float(np.float32(mean)), float(np.float32(std))
    return fb.kaldi_ref_bound(torch.from_numpy(af.kaldi_fbank(np.asarray(wav, dtype=np.float32), m32, s32, as_f64=True)))


def patches_of(fbank_clip, T):
    """fbank [frames, 128] f32 -> the clip's T patch rows, exact: row 8 t' + f', column 16 i + j = bf16(fbank[16 t' + i][16 f' + j])."""
    return fbank_clip[:2 * T].reshape(T // 8, 16, 8, 16).permute(0, 2, 1, 3).reshape(T, 256).to(BF16)


def posconv_weight(sd, p):
    """weight_norm(dim=2) of the positional conv in f32 on the CPU, exactly as beats_encoder takes it: [d, d / groups, 128] f32."""
    g, v = sd[p + "encoder.pos_conv.0.weight_g"].float().cpu(), sd[p + "encoder.pos_conv.0.weight_v"].float().cpu()
    return v * (g / v.norm(dim=(0, 1), keepdim=True))


def rel_table(sd, p, span, cfg):
    return om.beats_position_bias_table({k: v.cpu() for k, v in sd.items() if "relative_attention_bias" in k}, span, p,
                                        cfg.num_buckets, cfg.max_distance)


def check_packed_beats(sd, w, p):
    c = w.cfg
    pw = sd[p + "patch_embedding.weight"].float().to(BF16)
    assert same_bits(w.patch_w, pw.reshape(c.embed, 256)), "packing: patch_w is not patch_embedding.weight, row-major 16 x 16"
    wn = posconv_weight(sd, p).to(BF16)                                  # [d, cpg, 128]
    G, cpg = c.conv_groups, c.d_model // c.conv_groups
    want = wn.view(G, cpg, cpg, c.conv_pos).permute(0, 1, 3, 2).reshape(G, cpg, c.conv_pos * cpg)
    assert same_bits(w.posconv_w, want), "packing: posconv_w is not the tap-major bf16 image of the weight-normed pos_conv"
    assert same_bits(w.rel_table, rel_table(sd, p, w.rel_span, c)), "packing: rel_table is not the bucketed bias table"


def patch_embed(sd, p, patches):
    """patches [M, 256] bf16 -> the 16 x 16 / stride 16 Conv2d (no bias), [M, embed]."""
    w = _w(sd, p + "patch_embedding.weight", patches.device)
    dot, mag = fb.dot64(patches, w.reshape(w.shape[0], 256))
    return fb.gemm_ref_bound(dot, mag, 256)


def posconv(sd, p, xm, groups):
    """xm [T, d] f32 (one clip, padded rows zeroed) -> xm + GELU(conv1d(bf16(xm), padding 64, groups)[:T]) (SamePad drops
    the last of the T + 1 frames)."""
    dev = xm.device
    T, d = xm.shape
    cpg = d // groups
    w = rnd64(posconv_weight(sd, p)).to(dev)
    xb = rnd64(xm)
    dots, mags = [], []
    for g in range(groups):
        dot, mag = conv1d64(xb[None, :, g * cpg:(g + 1) * cpg], w[g * cpg:(g + 1) * cpg], 1, 64)
        dots.append(dot[0, :T])
        mags.append(mag[0, :T])
    return fb.gemm_ref_bound(torch.cat(dots, 1), torch.cat(mags, 1), 128 * cpg, bias=_p(sd, p + "encoder.pos_conv.0.bias", dev),
                             residual=xm, gelu=True)


def beats_gate(sd, lp, q, n_heads):
    """q [M, C] bf16 (the projected, unscaled queries) -> the gate of the relative position bias [M, H]."""
    dev = q.device
    return fb.gate_ref_bound(q.reshape(q.shape[0], n_heads, -1), _p(sd, lp + "self_attn.grep_linear.weight", dev),
                             _p(sd, lp + "self_attn.grep_linear.bias", dev), _p(sd, lp + "self_attn.grep_a", dev).reshape(-1))


# ---------------------------------------------------------------------------------------------------------------------------
# window-level Q-Former (K6, K7, K8)
# ---------------------------------------------------------------------------------------------------------------------------
QF = "speech_Qformer.bert."


def window_shape(T, second_per_window, second_stride):
    return om.salmonn_window_count(T, second_per_window, second_stride)


def window_attention(q, kv, n_clips, T, win, n_win, n_heads):
    """q [n_clips n_win, C] (one query per window), kv [n_clips T, 2 C] (keys | values of every frame): window w of clip a
    attends frames [win w, win w + win) of that clip."""
    C = q.shape[1]
    return oa.qformer_ref(q, kv, C, n_clips, n_win, win, T, n_heads, (C // n_heads) ** -0.5)

"""A torch emulation of every runtime.binding wrapper the audio encoder engines call, so that the engines of runtime/engines.py
run on CPU tensors (tests/test_encoder_stages.py).  Not a test module and not a conftest.

Each emulation is computed from the launch's ARGUMENTS alone, the way the kernel reads them: operands and results are
``as_strided`` views over the argument's storage with the leading dimensions, batch strides, row and column counts the launch
passes (``lda``, ``batch``, ``stride_a``, ``stride_c``, ``stride_r``, the offsets of column views, ``N=``, ``M=``, ``K=``), so a
wrong stride, offset or count in the host code moves what the emulation reads and writes exactly as it would move the kernel.
The arithmetic is float64 rounded once to the kernel's f32 value, and once more to bf16 where the kernel stores bf16.

``installed(mutate)`` puts the emulations in place of the wrappers; ``mutate(name, ordinal, arguments)`` (optional; ordinal counts
the launches of that wrapper, arguments is the dict of the launch's bound arguments) may alter the arguments of a launch before
its emulation sees them: the planted mistakes of test_encoder_stages.py."""
import contextlib
import functools
import inspect
import math

import numpy as np
import torch

from oracle import audio_frontend as af

BF16, F32 = torch.bfloat16, torch.float32


def _rows(t, batch, M, N, ld, stride):
    """[batch, M, N] over t's storage from t's first element: row pitch ld, batch pitch stride (elements)."""
    return torch.as_strided(t, (batch, M, N), (stride, ld, 1), t.storage_offset())


def _store(dst, val64):
    dst.copy_(val64.to(F32).to(dst.dtype))


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gemm(a, w, out, *, bias=None, residual=None, gelu=False, swiglu=False, split_k=1, workspace=None, tile=0, M=None, K=None,
         lda=None, batch=1, stride_a=0, stride_c=0, stride_r=0, rope=None, N=None, w_scale=None):
    assert not swiglu and rope is None and w_scale is None and split_k == 1
    N = w.shape[0] if N is None else N
    M = a.shape[-2] if M is None else M
    K = w.shape[1] if K is None else K
    lda = a.stride(-2) if lda is None else lda
    A = _rows(a, batch, M, K, lda, stride_a).double()
    W = torch.as_strided(w, (N, K), (w.stride(0), 1), w.storage_offset()).double()
    c = A @ W.t()
    if bias is not None:
        c = c + bias[:N].double()
    if gelu:
        c = _gelu(c)
    if residual is not None:
        c = c + _rows(residual, batch, M, N, residual.stride(-2), stride_r).double()
    _store(_rows(out, batch, M, N, out.stride(-2), stride_c), c)
    return out


def layernorm(x, gamma, beta, out, eps, *, res=None, alpha=1.0, out2=None, M=None, N=None):
    M = x.shape[0] if M is None else M
    N = x.shape[1] if N is None else N
    z = _rows(x, 1, M, N, x.stride(0), 0)[0].double()
    if res is not None:
        z = z + float(np.float32(alpha)) * _rows(res, 1, M, N, x.stride(0), 0)[0].double()
    d = z - z.mean(-1, keepdim=True)
    y = (d * torch.rsqrt(d.pow(2).mean(-1, keepdim=True) + eps) * gamma[:N].double() + beta[:N].double()).to(F32)
    _rows(out, 1, M, N, out.stride(0), 0)[0].copy_(y.to(out.dtype))
    if out2 is not None:
        _rows(out2, 1, M, N, out2.stride(0), 0)[0].copy_(y.to(out2.dtype))
    return out


def attn_fwd(q, k, v, out, cu_seqlens, max_seqlen, n_heads, head_dim, scale, *, causal=False, kv_lens=None, rel_bias=None,
             rel_gate=None, rel_span=0, kv_cache_max_len=0, cu_q=None, n_kv_heads=0):
    assert not causal and kv_cache_max_len == 0 and cu_q is None and n_kv_heads == 0
    H, D = n_heads, head_dim
    cu = cu_seqlens.tolist()
    for s in range(len(cu) - 1):
        a, L = cu[s], cu[s + 1] - cu[s]
        if L <= 0:
            continue
        assert L <= max_seqlen
        g = lambda t: _rows(t, 1, a + L, H * D, t.stride(0), 0)[0, a:].reshape(L, H, D).transpose(0, 1).double()
        sc = scale * (g(q) @ g(k).transpose(-1, -2))                    # [H, L, L]
        i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
        if rel_bias is not None:
            idx = (j - i).clamp(-(rel_span - 1), rel_span - 1) + rel_span - 1
            gate = torch.as_strided(rel_gate, (a + L, H), (H, 1), rel_gate.storage_offset())[a:]
            sc = sc + gate.double().t()[:, :, None] * rel_bias.double()[:, idx]
        kvl = L if kv_lens is None else min(max(int(kv_lens[s]), 1), L)
        sc = sc.masked_fill((j >= kvl)[None], float("-inf"))
        o = torch.softmax(sc, -1) @ g(v)
        _store(_rows(out, 1, a + L, H * D, out.stride(0), 0)[0, a:], o.transpose(0, 1).reshape(L, H * D))
    return out


def qformer_window_xattn(q, kv, v_off, out, n_audio, win_per_audio, win, rows_per_audio, n_heads, scale):
    H, D = n_heads, 64
    W = n_audio * win_per_audio
    qq = _rows(q, 1, W, H * D, q.stride(0), 0)[0].reshape(W, H, 1, D).double()
    kvv = _rows(kv, 1, n_audio * rows_per_audio, v_off + H * D, kv.stride(0), 0)[0]
    r0 = (torch.arange(W) // win_per_audio) * rows_per_audio + (torch.arange(W) % win_per_audio) * win
    rows = r0[:, None] + torch.arange(win)[None]                        # [W, win]
    kk = kvv[rows][..., :H * D].reshape(W, win, H, D).transpose(1, 2).double()
    vv = kvv[rows][..., v_off:v_off + H * D].reshape(W, win, H, D).transpose(1, 2).double()
    o = torch.softmax(scale * (qq @ kk.transpose(-1, -2)), -1) @ vv     # [W, H, 1, D]
    _store(_rows(out, 1, W, H * D, out.stride(0), 0)[0], o.reshape(W, H * D))


def beats_gate(qkv, grep_w, grep_b, grep_a, gate, n_heads, M=None):
    M = qkv.shape[0] if M is None else M
    q = _rows(qkv, 1, M, n_heads * 64, qkv.stride(0), 0)[0].reshape(M, n_heads, 64).double()
    s = (q @ grep_w.double().t() + grep_b.double()).view(M, n_heads, 2, 4).sum(-1)
    sa, sb = torch.sigmoid(s[..., 0]), torch.sigmoid(s[..., 1])
    _store(torch.as_strided(gate, (M, n_heads), (n_heads, 1), gate.storage_offset()), sa * (sb * grep_a.double() - 1.0) + 2.0)


def axpby_cast(x, out, alpha=1.0, add=None):
    M, N = x.shape
    y = torch.as_strided(x, (M, N), (x.stride(0), 1), x.storage_offset()).double() * float(np.float32(alpha))
    if add is not None:
        y = y + torch.as_strided(add, (M, N), (add.stride(0), 1), add.storage_offset()).double()
    _store(torch.as_strided(out, (M, N), (out.stride(0), 1), out.storage_offset()), y)
    return out


def _xt_fill(xt, spec32):
    n, n_mel, T = spec32.shape
    ld = xt.stride(-2)
    v = torch.as_strided(xt, (n, T + 2, ld), (xt.stride(0), ld, 1), xt.storage_offset())
    v.zero_()
    v[:, 1:T + 1, :n_mel] = spec32.transpose(1, 2).to(BF16)


def logmel_whisper(wav, wav_lens, mel_filters, n_mel, spec, xt, workspace):
    s = torch.stack([torch.from_numpy(af.whisper_logmel(wav[b, :int(L)].numpy(), n_mel, filters=mel_filters.numpy(), as_f64=True))
                     for b, L in enumerate(wav_lens.tolist())]).to(F32)
    if spec is not None:
        spec.copy_(s)
    if xt is not None:
        _xt_fill(xt, s)


def spec_to_xt(spec, xt):
    _xt_fill(xt, spec)


def fbank_kaldi(wav, wav_lens, mel_banks, max_frames, mean, std, out):
    m32, s32 = float(np.float32(mean)), float(np.float32(std))
    o = torch.as_strided(out, (wav.shape[0], max_frames, 128), (max_frames * 128, 128, 1), out.storage_offset())
    for b, L in enumerate(wav_lens.tolist()):
        r = torch.from_numpy(af.kaldi_fbank(wav[b, :int(L)].numpy(), m32, s32, as_f64=True))[:max_frames]
        o[b, :r.shape[0]] = r.to(F32)


def _flat(t, n):
    return torch.as_strided(t, (n,), (1,), t.storage_offset())


def beats_patchify(fbank, cu_rows, total_rows, out):
    max_frames, n = fbank.shape[1], fbank.shape[0]
    cu = cu_rows.tolist()
    row = torch.arange(total_rows)
    a = (torch.bucketize(row, torch.tensor(cu[1:n]), right=True) if n > 1 else torch.zeros_like(row))
    local = row - torch.tensor(cu)[a]
    tp, fp = local // 8, local % 8
    i, j = torch.arange(16)[:, None], torch.arange(16)[None, :]
    src = ((a * max_frames + tp * 16)[:, None, None] + i) * 128 + (fp * 16)[:, None, None] + j     # [rows, 16, 16] flat offsets
    assert int(src.min()) >= 0 and int(src.max()) < fbank.numel(), "beats_patchify would read outside the fbank buffer"
    _flat(out, total_rows * 256).copy_(_flat(fbank, fbank.numel())[src.reshape(-1)].to(BF16))


def beats_posconv_pack(x, cu_rows, valid_rows, n_audio, total_rows, groups, xg):
    C = x.shape[1]
    cpg = C // groups
    cu, valid = cu_rows.tolist(), valid_rows.tolist()
    xf = _flat(x, total_rows * C).view(total_rows, C)
    g = _flat(xg, (total_rows + 128 * n_audio) * C)
    for a in range(n_audio):
        T = cu[a + 1] - cu[a]
        xa = xf[cu[a]:cu[a + 1]]
        xa[min(max(valid[a], 0), T):] = 0
        img = torch.zeros(groups, T + 128, cpg, dtype=BF16)
        img[:, 64:64 + T] = xa.to(BF16).view(T, groups, cpg).transpose(0, 1)
        base = (cu[a] + 128 * a) * C
        g[base:base + (T + 128) * C].copy_(img.reshape(-1))


EMULATIONS = dict(gemm=gemm, layernorm=layernorm, attn_fwd=attn_fwd, qformer_window_xattn=qformer_window_xattn,
                  beats_gate=beats_gate, axpby_cast=axpby_cast, logmel_whisper=logmel_whisper, spec_to_xt=spec_to_xt,
                  fbank_kaldi=fbank_kaldi, beats_patchify=beats_patchify, beats_posconv_pack=beats_posconv_pack)


@contextlib.contextmanager
def installed(mutate=None):
    """runtime.binding's encoder wrappers replaced by the emulations (restored on exit)."""
    import icl_speech_text_llm_amd.runtime.binding as B
    saved = {n: getattr(B, n) for n in EMULATIONS}
    counts = {n: 0 for n in EMULATIONS}

    def wrap(name, emu):
        sig = inspect.signature(emu)

        @functools.wraps(emu)
        def call(*args, **kwargs):
            k = counts[name]
            counts[name] += 1
            ba = sig.bind(*args, **kwargs)
            if mutate is not None:
                mutate(name, k, ba.arguments)          # edits the launch's arguments in place
            return emu(*ba.args, **ba.kwargs)
        return call

    try:
        for n, emu in EMULATIONS.items():
            setattr(B, n, wrap(n, emu))
        yield
    finally:
        for n, f in saved.items():
            setattr(B, n, f)

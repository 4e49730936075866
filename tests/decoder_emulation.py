"""A torch emulation of every runtime.binding wrapper the LLM decoder (LlamaHIP of runtime/engines.py) calls, so that prefill,
the trimmed last layer, decode_step and logits run on CPU tensors (tests/test_decoder_stages.py).  Not a test module and not a
conftest.

As in tests/encoder_emulation.py, each emulation is computed from the launch's ARGUMENTS alone, the way the kernel reads them:
operands and results are ``as_strided`` views over the argument's storage with the leading dimensions, column offsets, row
counts (``M=`` / ``N=`` / ``K=``), ``pos`` / ``seq_ids`` / ``lens``, ``max_len`` and head counts the launch passes — a cache is
addressed as ((seq n_kv_heads + head) max_len + pos) head_dim from the argument's first element, whatever the tensor's shape
says — so a wrong offset, count or plane in the host code moves what the emulation reads and writes exactly as it would move the
kernel.  Tile, split-K and workspace arguments are accepted and ignored.  The arithmetic is float64 rounded once to the kernel's
f32 value, and once more to bf16 where the kernel stores bf16; FP8 rows go through tests/fp8_ref.py.  The fused launches (GEMM
with the RoPE epilogue, attn_decode_rope*) are their two-launch form, which is their contract.

``installed()`` puts the emulations in place of the wrappers.  The planted mistakes of test_decoder_stages.py alter a launch's
arguments one level up, in the recorder of tests/decoder_stage_check.py (``recording(mutate)``): recorder and emulation then see
the launch exactly as mistaken host code would have made it."""
import contextlib

import torch

import encoder_emulation as enc
import fp8_ref

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8


def _mat(t, M, N, ld=None):
    return torch.as_strided(t, (M, N), (t.stride(0) if ld is None else ld, 1), t.storage_offset())


def _flat(t):
    """Everything from t's first element to the end of its storage."""
    n = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
    return torch.as_strided(t, (n,), (1,), t.storage_offset())


def _cache(t, n_kv_heads, max_len, D, width=None):
    """A cache plane addressed from its first element: [seqs, n_kv_heads, max_len, D] (``width=1``: a scale plane, no D)."""
    flat = _flat(t)
    row = D if width is None else 1
    seqs = flat.numel() // (n_kv_heads * max_len * row)
    v = flat[:seqs * n_kv_heads * max_len * row]
    return v.view(seqs, n_kv_heads, max_len, D) if width is None else v.view(seqs, n_kv_heads, max_len)


def _bf(x64):
    return x64.to(F32).to(BF16)


def _unpack_fp8(q, N, K):
    """The row-major bytes of an fp8 decode-packed copy (the inverse of fp8_ref.ref_pack)."""
    Np = q.shape[0]
    return q.reshape(Np // 16, K // 64, 4, 16, 2, 8).permute(0, 3, 1, 4, 2, 5).reshape(Np, K)[:N]


def _weight(w, N, K, w_scale):
    if w_scale is None:
        return torch.as_strided(w, (N, K), (w.stride(0), 1), w.storage_offset()).double()
    return _unpack_fp8(w, N, K).view(torch.float8_e4m3fn).double() * w_scale[:N].double()[:, None]


def _rot(x, cos, sin, pos):
    """x [M, heads, D] -> rotate-half at cos / sin [pos[m]], float64."""
    h = x.shape[-1] // 2
    c, s = cos[pos.long()].double()[:, None, :h], sin[pos.long()].double()[:, None, :h]
    a, b = x[..., :h].double(), x[..., h:].double()
    return torch.cat([a * c - b * s, b * c + a * s], -1)


def _head_norm(x, gamma, eps):
    x = x.double()
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + float(torch.tensor(eps, dtype=F32))) * gamma.double()


def _rope_append(qkv, k_off, v_off, cos, sin, pos, seq_ids, kc, vc, H, Hkv, D, max_len, M, *, gammas=None, eps=0.0,
                 rotate_k_in_place=True, fp8=None, rotate=True, has_q=True, has_kv=True):
    """The one head-row kernel in all its forms, over qkv rows addressed by the argument's own leading dimension."""
    ld = qkv.stride(0)
    blk = lambda off, n: torch.as_strided(qkv, (M, n, D), (ld, D, 1), qkv.storage_offset() + off)
    q = blk(0, H) if has_q else None
    k, v = (blk(k_off, Hkv), blk(v_off, Hkv)) if has_kv else (None, None)
    kr = None
    if rotate:
        if q is not None:
            qn = _bf(_head_norm(q, gammas[0], eps)) if gammas is not None else q
            q.copy_(_bf(_rot(qn, cos, sin, pos)))
        if k is not None:
            kn = _bf(_head_norm(k, gammas[1], eps)) if gammas is not None else k
            kr = _bf(_rot(kn, cos, sin, pos))
            if rotate_k_in_place:
                k.copy_(kr)
    elif k is not None:
        kr = k.clone()
    s = torch.arange(M) if seq_ids is None else seq_ids.long()
    p, hh = pos.long(), torch.arange(Hkv)
    if fp8 is not None:
        kq, vq, ks, vs = fp8
        for rows, cq, cs in ((kr, kq, ks), (v, vq, vs)):
            b, sc, _ = fp8_ref.ref_q(rows)
            _cache(cq, Hkv, max_len, D)[s[:, None], hh[None], p[:, None]] = b
            _cache(cs, Hkv, max_len, D, width=1)[s[:, None], hh[None], p[:, None]] = sc
    elif kc is not None:
        _cache(kc, Hkv, max_len, D)[s[:, None], hh[None], p[:, None]] = kr
        _cache(vc, Hkv, max_len, D)[s[:, None], hh[None], p[:, None]] = v.clone()


def gemm(a, w, out, *, bias=None, residual=None, gelu=False, swiglu=False, split_k=1, workspace=None, tile=0, M=None, K=None,
         lda=None, batch=1, stride_a=0, stride_c=0, stride_r=0, rope=None, N=None, w_scale=None):
    if not swiglu and rope is None and w_scale is None:
        return enc.gemm(a, w, out, bias=bias, residual=residual, gelu=gelu, M=M, K=K, lda=lda, batch=batch, stride_a=stride_a,
                        stride_c=stride_c, stride_r=stride_r, N=N)
    assert batch == 1 and not gelu
    N = w.shape[0] if N is None else N
    M = a.shape[-2] if M is None else M
    K = w.shape[1] if K is None else K
    c = _mat(a, M, K, lda).double() @ _weight(w, N, K, w_scale).t()
    if bias is not None:
        c = c + bias[:N].double()
    if swiglu:
        g = c.reshape(M, N // 32, 2, 16)
        c = (g[:, :, 0] * torch.sigmoid(g[:, :, 0]) * g[:, :, 1]).reshape(M, N // 2)
        _mat(out, M, N // 2).copy_(c.to(F32).to(out.dtype))
        return out
    if residual is not None:
        c = c + _mat(residual, M, N).double()
    if rope is None:
        _mat(out, M, N).copy_(c.to(F32).to(out.dtype))
        return out
    k_off, v_off, cos, sin, pos, seq_ids, kc, vc, H, D, max_len = rope[:11]
    to_c = bool(rope[11]) if len(rope) > 11 else True
    tmp = _bf(c).contiguous()                                 # the bf16 C the two-launch form rotates
    Hq, Hk = k_off // D, (v_off - k_off) // D
    Hk = Hk if N > v_off else 0
    _rope_append(tmp, k_off, v_off, cos, sin, pos, seq_ids, kc, vc, Hq, Hk, D, max_len, M, has_q=Hq > 0, has_kv=N > v_off)
    cols = N if to_c else k_off
    if cols:
        _mat(out, M, cols).copy_(tmp[:, :cols])
    return out


def gemm_rmsnorm(a, w, out, gamma, eps, xn, *, residual=None, split_k=1, workspace=None, tile=0, N=None, K=None, w_scale=None):
    N = w.shape[0] if N is None else N
    K = w.shape[1] if K is None else K
    M = a.shape[-2]
    c = _mat(a, M, K).double() @ _weight(w, N, K, w_scale).t()
    if residual is not None:
        c = c + _mat(residual, M, N).double()
    c32 = c.to(F32)
    _mat(out, M, N).copy_(c32)
    z = c32.double()
    _mat(xn, M, N).copy_(_bf(z * torch.rsqrt(z.pow(2).mean(-1, keepdim=True) + eps) * gamma[:N].double()))
    return out


def rmsnorm(x, gamma, out, eps, *, M=None, N=None):
    M = x.shape[0] if M is None else M
    N = x.shape[1] if N is None else N
    z = _mat(x, M, N).double()
    _mat(out, M, N).copy_((z * torch.rsqrt(z.pow(2).mean(-1, keepdim=True) + eps) * gamma[:N].double()).to(F32).to(out.dtype))
    return out


def lora_down(x, K0, a, r_total, scale, M=None):
    M = x.shape[0] if M is None else M
    A = torch.as_strided(a, (r_total, K0), (a.stride(0), 1), a.storage_offset()).double()
    t = float(torch.tensor(scale, dtype=F32)) * (_mat(x, M, K0).double() @ A.t())
    torch.as_strided(x, (M, r_total), (x.stride(0), 1), x.storage_offset() + K0).copy_(_bf(t))


def rope_kv(qkv, k_off, v_off, cos, sin, pos, seq_ids, kcache, vcache, n_heads, head_dim, max_len, M=None):
    M = qkv.shape[0] if M is None else M
    _rope_append(qkv, k_off, v_off, cos, sin, pos, seq_ids, kcache, vcache, n_heads, n_heads, head_dim, max_len, M)


def rope_kv_gqa(qkv, k_off, v_off, cos, sin, pos, seq_ids, kcache, vcache, n_heads, n_kv_heads, head_dim, max_len, M=None):
    M = qkv.shape[0] if M is None else M
    _rope_append(qkv, k_off, v_off, cos, sin, pos, seq_ids, kcache, vcache, n_heads, n_kv_heads, head_dim, max_len, M)


def qknorm_rope_kv(qkv, k_off, v_off, q_gamma, k_gamma, eps, cos, sin, pos, seq_ids, kcache, vcache, n_heads, n_kv_heads,
                   head_dim, max_len, M=None):
    M = qkv.shape[0] if M is None else M
    _rope_append(qkv, k_off, v_off, cos, sin, pos, seq_ids, kcache, vcache, n_heads, n_kv_heads, head_dim, max_len, M,
                 gammas=(q_gamma, k_gamma), eps=eps)


def rope_kv_fp8(qkv, k_off, v_off, cos, sin, pos, seq_ids, kq, vq, ks, vs, n_heads, head_dim, max_len, M=None):
    M = qkv.shape[0] if M is None else M
    _rope_append(qkv, k_off, v_off, cos, sin, pos, seq_ids, None, None, n_heads, n_heads, head_dim, max_len, M,
                 rotate_k_in_place=False, fp8=(kq, vq, ks, vs))


def kv_append_fp8(qkv, k_off, v_off, pos, seq_ids, kq, vq, ks, vs, n_heads, head_dim, max_len, M=None):
    M = qkv.shape[0] if M is None else M
    _rope_append(qkv, k_off, v_off, None, None, pos, seq_ids, None, None, n_heads, n_heads, head_dim, max_len, M,
                 fp8=(kq, vq, ks, vs), rotate=False, has_q=False)


def _softmax_rows(q, k, v, scale, first_pos):
    """q [H, Lq, D], k / v [H, L, D] float64; query i sees keys 0 .. first_pos + i."""
    Lq, L = q.shape[1], k.shape[1]
    sc = scale * (q @ k.transpose(-1, -2))
    hidden = torch.arange(L)[None, :] > (first_pos + torch.arange(Lq))[:, None]
    return torch.softmax(sc.masked_fill(hidden[None], float("-inf")), -1) @ v


def attn_fwd(q, k, v, out, cu_seqlens, max_seqlen, n_heads, head_dim, scale, *, causal=False, kv_lens=None, rel_bias=None,
             rel_gate=None, rel_span=0, kv_cache_max_len=0, cu_q=None, n_kv_heads=0):
    assert causal and kv_lens is None and rel_bias is None
    H, D, Hkv = n_heads, head_dim, n_kv_heads or n_heads
    cu = cu_seqlens.tolist()
    cq = cu if cu_q is None else cu_q.tolist()
    for s in range(len(cu) - 1):
        a, L, qa, Lq = cu[s], cu[s + 1] - cu[s], cq[s], cq[s + 1] - cq[s]
        if L <= 0 or Lq <= 0:
            continue
        assert L <= max_seqlen
        qq = torch.as_strided(q, (Lq, H, D), (q.stride(0), D, 1), q.storage_offset() + qa * q.stride(0)).transpose(0, 1).double()
        if kv_cache_max_len > 0:
            kk, vv = (_cache(t, Hkv, kv_cache_max_len, D)[s, :, :L].double() for t in (k, v))
        else:
            kk, vv = (torch.as_strided(t, (L, Hkv, D), (t.stride(0), D, 1), t.storage_offset() + a * t.stride(0))
                      .transpose(0, 1).double() for t in (k, v))
        kk, vv = kk.repeat_interleave(H // Hkv, 0), vv.repeat_interleave(H // Hkv, 0)
        o = _softmax_rows(qq, kk, vv, scale, L - Lq)
        torch.as_strided(out, (Lq, H * D), (out.stride(0), 1), out.storage_offset() + qa * out.stride(0)).copy_(
            _bf(o.transpose(0, 1).reshape(Lq, H * D)))
    return out


def _decode(q, keys, values, out, lens, H, Hkv, D, scale):
    """keys / values [seqs, Hkv, max_len, D] float64 (or anything .double() takes); row b attends its first lens[b] positions."""
    for b, L in enumerate(lens.tolist()):
        qq = torch.as_strided(q, (H, 1, D), (D, D, 1), q.storage_offset() + b * q.stride(0)).double()
        kk, vv = keys[b, :, :L].double().repeat_interleave(H // Hkv, 0), values[b, :, :L].double().repeat_interleave(H // Hkv, 0)
        o = torch.softmax(scale * (qq @ kk.transpose(-1, -2)), -1) @ vv
        torch.as_strided(out, (H * D,), (1,), out.storage_offset() + b * out.stride(0)).copy_(_bf(o.reshape(H * D)))
    return out


def attn_decode(q, kcache, vcache, out, lens, n_heads, head_dim, max_len, scale):
    return _decode(q, _cache(kcache, n_heads, max_len, head_dim), _cache(vcache, n_heads, max_len, head_dim), out, lens,
                   n_heads, n_heads, head_dim, scale)


def attn_decode_gqa(q, kcache, vcache, out, lens, n_heads, n_kv_heads, head_dim, max_len, scale):
    return _decode(q, _cache(kcache, n_kv_heads, max_len, head_dim), _cache(vcache, n_kv_heads, max_len, head_dim), out, lens,
                   n_heads, n_kv_heads, head_dim, scale)


def _dequant(cq, cs, H, max_len, D, rows):
    q, s = _cache(cq, H, max_len, D)[:rows], _cache(cs, H, max_len, D, width=1)[:rows]
    return q.view(torch.float8_e4m3fn).double() * s.double()[..., None]


def attn_decode_fp8(q, kq, vq, ks, vs, out, lens, n_heads, head_dim, max_len, scale):
    n = lens.numel()
    return _decode(q, _dequant(kq, ks, n_heads, max_len, head_dim, n), _dequant(vq, vs, n_heads, max_len, head_dim, n), out, lens,
                   n_heads, n_heads, head_dim, scale)


def attn_decode_rope(qkv, k_off, v_off, cos, sin, pos, seq_ids, kcache, vcache, out, lens, n_heads, head_dim, max_len, scale):
    tmp = _mat(qkv, qkv.shape[0], qkv.shape[1]).clone()            # qkv is left as the projection wrote it
    rope_kv(tmp, k_off, v_off, cos, sin, pos, seq_ids, kcache, vcache, n_heads, head_dim, max_len)
    return attn_decode(tmp[:, :k_off], kcache, vcache, out, lens, n_heads, head_dim, max_len, scale)


def attn_decode_rope_fp8(qkv, k_off, v_off, cos, sin, pos, seq_ids, kq, vq, ks, vs, out, lens, n_heads, head_dim, max_len, scale):
    tmp = _mat(qkv, qkv.shape[0], qkv.shape[1]).clone()
    rope_kv_fp8(tmp, k_off, v_off, cos, sin, pos, seq_ids, kq, vq, ks, vs, n_heads, head_dim, max_len)
    return attn_decode_fp8(tmp[:, :k_off], kq, vq, ks, vs, out, lens, n_heads, head_dim, max_len, scale)


def embed_gather_interleave(src_idx, table, speech, out):
    H = table.shape[1]
    o = torch.as_strided(out, (src_idx.numel(), H), (H, 1), out.storage_offset())      # the kernel has no leading dimension
    for r, s in enumerate(src_idx.tolist()):
        o[r] = table[s].float() if s >= 0 else torch.as_strided(speech, (H,), (1,), speech.storage_offset() + (-s - 1) * H)
    return out


def gather_rows(src, idx, out, N=None):
    N = src.shape[1] if N is None else N
    n = idx.numel()
    rows = torch.as_strided(src, (int(idx.max()) + 1, N), (src.stride(0), 1), src.storage_offset())[idx.long()]
    _mat(out, n, N).copy_(rows)
    return out


def pack_decode_weights(w, K=None):
    N, K = w.shape[0], (w.shape[1] if K is None else K)
    out = torch.zeros((N + 15) // 16 * 16, K, dtype=BF16)
    out[:N] = w[:, :K]
    return out


def pack_fp8_weights(w, K=None, out=None):
    K = w.shape[1] if K is None else K
    q, s, wp = fp8_ref.ref_q(w[:, :K])
    if out is not None:
        out[:, :K] = wp
    return fp8_ref.ref_pack(q), s, wp if out is None else out


EMULATIONS = dict(gemm=gemm, gemm_rmsnorm=gemm_rmsnorm, rmsnorm=rmsnorm, lora_down=lora_down, rope_kv=rope_kv,
                  rope_kv_gqa=rope_kv_gqa, qknorm_rope_kv=qknorm_rope_kv, rope_kv_fp8=rope_kv_fp8, kv_append_fp8=kv_append_fp8,
                  attn_fwd=attn_fwd, attn_decode=attn_decode, attn_decode_gqa=attn_decode_gqa, attn_decode_fp8=attn_decode_fp8,
                  attn_decode_rope=attn_decode_rope, attn_decode_rope_fp8=attn_decode_rope_fp8,
                  embed_gather_interleave=embed_gather_interleave, gather_rows=gather_rows)
HOST = dict(pack_decode_weights=pack_decode_weights, pack_fp8_weights=pack_fp8_weights)     # no launches of the chain: never mutated


@contextlib.contextmanager
def installed():
    """runtime.binding's decoder wrappers replaced by the emulations (restored on exit)."""
    import icl_speech_text_llm_amd.runtime.binding as B
    saved = {n: getattr(B, n) for n in list(EMULATIONS) + list(HOST)}
    try:
        for n, f in list(EMULATIONS.items()) + list(HOST.items()):
            setattr(B, n, f)
        yield
    finally:
        for n, f in saved.items():
            setattr(B, n, f)

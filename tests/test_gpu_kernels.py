"""Parity of every libicl_hip kernel against a plain PyTorch fp32 reference of the same op
(`-m gpu`; all calls go through the C-ABI via runtime/binding.py)."""
import math

import numpy as np
import pytest
import torch

from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _rand_bf16(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(DEV)


def _relerr(got, ref):
    got, ref = got.float(), ref.float()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


# ------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------
GEMM_SHAPES = [
    (128, 128, 64), (256, 384, 128), (300, 200, 192), (1, 64, 64), (33, 4096, 4096 // 8), (1500, 1280, 1280),
    (376, 4096, 4096), (88, 768, 3072), (17, 48, 6144),
]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES + [(512, 512, 64), (700, 1000, 448), (6016, 768, 2048)])
@pytest.mark.parametrize("tile", [1, 2, 3])
def test_gemm_plain(B, M, N, K, tile):
    a, w = _rand_bf16(M, K, seed=1), _rand_bf16(N, K, seed=2)
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    B.gemm(a, w, out, tile=tile)
    ref = a.float() @ w.float().t()
    torch.cuda.synchronize()
    err = (out - ref).abs().max().item()
    assert err <= 1e-3 * math.sqrt(K), (err, M, N, K)
    assert _relerr(out, ref) < 1e-5


@pytest.mark.parametrize("K", [256, 512, 1280])
def test_gemm_many_tiles_all_epilogues(B, K):
    """256x256 kernel over a grid of 616 tiles (2-3 per CU), every epilogue; the all-interior launch is bit-compared with a
    launch whose extra row adds an edge row-tile (a row's arithmetic must not depend on how the grid is cut)."""
    M, N = 256 * 44, 256 * 14                     # 616 tiles
    a, w = _rand_bf16(M + 1, K, seed=11, scale=0.5), _rand_bf16(N, K, seed=12, scale=0.1)
    bias = torch.randn(N, device=DEV)
    res32 = torch.randn(M + 1, N, device=DEV)
    res16 = _rand_bf16(M + 1, N, seed=13)
    base = a[:M].float() @ w.float().t()

    def both(out_dtype, n_out=N, **kw):
        outs = []
        for rows in (M, M + 1):
            out = torch.full((rows, n_out), float("nan"), dtype=out_dtype, device=DEV)
            r = kw.get("residual")
            B.gemm(a[:rows], w, out, tile=3, **{**kw, **({"residual": r[:rows]} if r is not None else {})})
            outs.append(out[:M])
        assert torch.equal(outs[0], outs[1]), kw.keys()
        return outs[0]

    out = both(torch.float32)
    assert (out - base).abs().max().item() <= 1e-3 * math.sqrt(K) and _relerr(out, base) < 1e-5
    out = both(torch.bfloat16, bias=bias, gelu=True)
    assert _relerr(out, torch.nn.functional.gelu(base + bias)) < 4e-3
    out = both(torch.float32, bias=bias, residual=res32)
    assert (out - (base + bias + res32[:M])).abs().max().item() <= 2e-3
    out = both(torch.bfloat16, residual=res16)
    assert _relerr(out, base + res16[:M].float()) < 4e-3
    out = both(torch.float32, bias=bias, gelu=True, residual=res32)
    assert (out - (torch.nn.functional.gelu(base + bias) + res32[:M])).abs().max().item() <= 2e-3
    out = both(torch.bfloat16, n_out=N // 2, swiglu=True)
    g = base.view(M, N // 32, 2, 16)
    assert _relerr(out, (torch.nn.functional.silu(g[:, :, 0]) * g[:, :, 1]).reshape(M, N // 2)) < 4e-3
    # in-place residual stream (the way the engines call it)
    stream = res32[:M].clone()
    B.gemm(a[:M], w, stream, bias=bias, residual=stream, tile=3)
    assert (stream - (base + bias + res32[:M])).abs().max().item() <= 2e-3


def test_gemm_identity_asymmetric(B):
    # A = I with an asymmetric W catches a transposed C write (guide §3)
    K = 128
    a = torch.eye(K, dtype=torch.bfloat16, device=DEV)
    w = (torch.arange(256 * K, device=DEV).reshape(256, K) % 251).to(torch.bfloat16)
    out = torch.empty(K, 256, dtype=torch.float32, device=DEV)
    B.gemm(a, w, out)
    assert torch.equal(out, w.float().t())


@pytest.mark.parametrize("tile", [1, 2, 3])
def test_gemm_epilogues(B, tile):
    M, N, K = 200, 256, 256
    a, w = _rand_bf16(M, K, seed=3, scale=0.5), _rand_bf16(N, K, seed=4, scale=0.1)
    bias = torch.randn(N, device=DEV)
    res32 = torch.randn(M, N, device=DEV)
    res16 = _rand_bf16(M, N, seed=5)
    base = a.float() @ w.float().t()
    # bias + gelu -> bf16
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    B.gemm(a, w, out, bias=bias, gelu=True, tile=tile)
    ref = torch.nn.functional.gelu(base + bias)
    assert (out.float() - ref).abs().max().item() <= 2e-2 and _relerr(out, ref) < 4e-3
    # bias + f32 residual -> f32 (in place on the residual stream)
    stream = res32.clone()
    B.gemm(a, w, stream, bias=bias, residual=stream, tile=tile)
    assert (stream - (base + bias + res32)).abs().max().item() <= 1e-3
    # bf16 residual -> bf16
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    B.gemm(a, w, out, residual=res16, tile=tile)
    ref = base + res16.float()
    assert _relerr(out, ref) < 4e-3
    # gelu then residual (Whisper conv2 + positional embedding order)
    out = torch.empty(M, N, dtype=torch.float32, device=DEV)
    B.gemm(a, w, out, bias=bias, gelu=True, residual=res32, tile=tile)
    ref = torch.nn.functional.gelu(base + bias) + res32
    assert (out - ref).abs().max().item() <= 1e-3


@pytest.mark.parametrize("tile", [1, 2, 3])
@pytest.mark.parametrize("split_k", [1, 4])
def test_gemm_swiglu(B, tile, split_k):
    M, I, K = 70, 11008 // 8, 512
    a = _rand_bf16(M, K, seed=6, scale=0.5)
    wg, wu = _rand_bf16(I, K, seed=7, scale=0.1), _rand_bf16(I, K, seed=8, scale=0.1)
    # interleave gate/up rows in blocks of 16
    w = torch.stack([wg.view(I // 16, 16, K), wu.view(I // 16, 16, K)], dim=1).reshape(2 * I, K).contiguous()
    out = torch.empty(M, I, dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(split_k * M * 2 * I, dtype=torch.float32, device=DEV) if split_k > 1 else None
    B.gemm(a, w, out, swiglu=True, tile=tile, split_k=split_k, workspace=ws)
    ref = torch.nn.functional.silu(a.float() @ wg.float().t()) * (a.float() @ wu.float().t())
    assert _relerr(out, ref) < 4e-3


@pytest.mark.parametrize("M,N,K,split", [(256, 1024, 4160, 5), (256, 512, 4096, 16), (200, 768, 11008, 16), (130, 1000, 832, 3)])
def test_gemm_256_tile_split_k(B, M, N, K, split):
    """Split-K on the 256x256 tile (decode at 129..256 rows: one M-tile and too few N-tiles to fill the chip): uneven K slices,
    edge tiles in M and N, the slabs reduced by the same kernels as the other tiles' — incl. the fused reduce + residual +
    RMSNorm — so the f32 row must equal tile 2's for the same split (same slab boundaries, same summation order of the slabs;
    inside a slab the k order differs by kernel: 1e-4)."""
    a, w = _rand_bf16(M, K, seed=41, scale=0.5), _rand_bf16(N, K, seed=42, scale=0.05)
    bias, res = torch.randn(N, device=DEV), torch.randn(M, N, device=DEV)
    ws = torch.empty(split * M * N, device=DEV)
    out = torch.empty(M, N, device=DEV)
    B.gemm(a, w, out, bias=bias, residual=res, tile=3, split_k=split, workspace=ws)
    ref = a.float() @ w.float().t() + bias + res
    assert (out - ref).abs().max().item() <= 2e-3
    out2 = torch.empty(M, N, device=DEV)
    B.gemm(a, w, out2, bias=bias, residual=res, tile=2, split_k=split, workspace=ws)
    assert (out - out2).abs().max().item() <= 1e-4
    gamma = 1.0 + 0.1 * torch.randn(N, device=DEV)
    h, xn = res.clone(), torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    B.gemm_rmsnorm(a, w, h, gamma, 1e-5, xn, residual=h, tile=3, split_k=split, workspace=ws)
    h2 = res.clone()
    B.gemm(a, w, h2, residual=h2, tile=3, split_k=split, workspace=ws)
    assert torch.equal(h, h2)
    assert _relerr(xn, torch.nn.functional.rms_norm(h2, (N,), gamma, 1e-5)) < 4e-3
    with pytest.raises(B.IclError):
        B.gemm(a, w, out, tile=3, split_k=K // 64, workspace=torch.empty(K // 64 * M * N, device=DEV))     # slices of one K-tile


@pytest.mark.parametrize("M", [1, 16, 32, 64])
@pytest.mark.parametrize("split_k", [2, 8])
def test_gemm_splitk_decode_shapes(B, M, split_k):
    N, K = 1024, 4096
    a, w = _rand_bf16(M, K, seed=9, scale=0.5), _rand_bf16(N, K, seed=10, scale=0.05)
    bias = torch.randn(N, device=DEV)
    res = torch.randn(M, N, device=DEV)
    out = torch.empty(M, N, dtype=torch.float32, device=DEV)
    ws = torch.empty(split_k * M * N, dtype=torch.float32, device=DEV)
    B.gemm(a, w, out, bias=bias, residual=res, split_k=split_k, workspace=ws, tile=2)
    ref = a.float() @ w.float().t() + bias + res
    assert (out - ref).abs().max().item() <= 2e-3


@pytest.mark.parametrize("tile", [0, 3])
def test_gemm_odd_n_unaligned_ldc(B, tile):
    # lm_head: N = 32001, ldc = 32001 (rows not 16-byte aligned -> scalar store path)
    M, N, K = 5, 32001, 256
    a, w = _rand_bf16(M, K, seed=11), _rand_bf16(N, K, seed=12, scale=0.05)
    out = torch.empty(M, N, dtype=torch.float32, device=DEV)
    B.gemm(a, w, out, tile=tile)
    ref = a.float() @ w.float().t()
    assert (out - ref).abs().max().item() <= 1e-3


@pytest.mark.parametrize("tile", [0, 3])
def test_gemm_conv_as_strided_gemm(B, tile):
    # Whisper conv2 (k=3, stride 2, pad 1) as a GEMM over a time-major padded operand with lda = 2*C
    Bn, T, C, Co = 2, 60, 64, 128
    x = _rand_bf16(Bn, T, C, seed=13)                       # [B, T, C] time-major
    wconv = _rand_bf16(Co, C, 3, seed=14, scale=0.1)        # torch Conv1d weight [Co, Ci, k]
    xp = torch.zeros(Bn, T + 2, C, dtype=torch.bfloat16, device=DEV)
    xp[:, 1:T + 1] = x
    wk = wconv.permute(0, 2, 1).reshape(Co, 3 * C).contiguous()   # [Co, k*C]
    Tout = T // 2
    out = torch.empty(Bn, Tout, Co, dtype=torch.float32, device=DEV)
    B.gemm(xp, wk, out, M=Tout, K=3 * C, lda=2 * C, batch=Bn, stride_a=(T + 2) * C, stride_c=Tout * Co, tile=tile)
    ref = torch.nn.functional.conv1d(x.float().transpose(1, 2), wconv.float(), stride=2, padding=1).transpose(1, 2)
    assert (out - ref).abs().max().item() <= 2e-3


def test_gemm_rejects_bad_args(B):
    a, w = _rand_bf16(8, 96), _rand_bf16(8, 96)
    out = torch.empty(8, 8, dtype=torch.float32, device=DEV)
    with pytest.raises(B.IclError, match="multiple of 64"):
        B.gemm(a, w, out)
    # the library stays usable after an error
    a, w = _rand_bf16(8, 64), _rand_bf16(8, 64)
    B.gemm(a, w, out)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
def _attn_ref(q, k, v, cu, H, D, scale, causal=False, kv_lens=None, rel_bias=None, rel_gate=None, rel_span=0):
    out = torch.zeros(q.shape[0], H * D, dtype=torch.float32, device=q.device)
    for s in range(len(cu) - 1):
        a, b = cu[s], cu[s + 1]
        L = b - a
        qs = q[a:b].float().view(L, H, D).transpose(0, 1)
        ks = k[a:b].float().view(L, H, D).transpose(0, 1)
        vs = v[a:b].float().view(L, H, D).transpose(0, 1)
        sc = qs @ ks.transpose(1, 2) * scale
        i = torch.arange(L, device=q.device)
        if rel_bias is not None:
            rel = (i[None, :] - i[:, None]).clamp(-(rel_span - 1), rel_span - 1) + rel_span - 1
            sc = sc + rel_gate[a:b].t()[:, :, None] * rel_bias[:, rel]
        mask = torch.zeros(L, L, dtype=torch.bool, device=q.device)
        if causal:
            mask |= i[None, :] > i[:, None]
        if kv_lens is not None:
            mask |= (i >= kv_lens[s])[None, :]
        sc = sc.masked_fill(mask[None], float("-inf"))
        o = torch.softmax(sc, dim=-1) @ vs
        out[a:b] = o.transpose(0, 1).reshape(L, H * D)
    return out


@pytest.mark.parametrize("D,H", [(64, 3), (128, 2)])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("lens", [[128], [1], [200, 64, 377], [1500]])
def test_attn_fwd(B, D, H, causal, lens):
    total = sum(lens)
    cu = [0]
    for L in lens:
        cu.append(cu[-1] + L)
    qkv = _rand_bf16(total, 3 * H * D, seed=21)
    q, k, v = qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:]
    out = torch.full((total, H * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    scale = D ** -0.5
    B.attn_fwd(q, k, v, out, cu_t, max(lens), H, D, scale, causal=causal)
    ref = _attn_ref(q, k, v, cu, H, D, scale, causal=causal)
    err = (out.float() - ref).abs().max().item()
    assert err <= 2e-2, err
    assert _relerr(out, ref) < 1e-2


def test_attn_fwd_d128_is_exact_up_to_the_output_rounding(B):
    """D = 128 (decoder prefill): P enters PV as a two-term bf16 split, so the kernel's bf16 output equals the f64 softmax-attention
    result ROUNDED to bf16 in all but a fraction of a percent of the elements (measured: 0.2 % differ, by one ulp) — the only
    rounding left is the one the oracle applies too (attention output -> bf16)."""
    D, H, L = 128, 2, 376
    qkv = _rand_bf16(L, 3 * H * D, seed=31)
    q, k, v = qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:]
    out = torch.empty(L, H * D, dtype=torch.bfloat16, device=DEV)
    cu_t = torch.tensor([0, L], dtype=torch.int32, device=DEV)
    B.attn_fwd(q, k, v, out, cu_t, L, H, D, D ** -0.5, causal=True)
    qs, ks, vs = (t.double().view(L, H, D).transpose(0, 1) for t in (q, k, v))
    sc = qs @ ks.transpose(1, 2) * D ** -0.5
    i = torch.arange(L, device=DEV)
    sc = sc.masked_fill((i[None, :] > i[:, None])[None], float("-inf"))
    exact = (torch.softmax(sc, -1) @ vs).transpose(0, 1).reshape(L, H * D)
    rounded = exact.to(torch.bfloat16)
    differ = float((out != rounded).double().mean())
    rel = float((out.double() - rounded.double()).norm() / exact.norm())
    print(f"attn D=128: {differ:.4f} of the elements differ from the rounded exact result, rel-L2 {rel:.2e}")
    assert differ < 0.01 and rel < 2e-4


@pytest.mark.parametrize("D,H,causal", [(128, 3, True), (64, 2, False)])
def test_attn_fwd_reads_kv_from_cache_layout(B, D, H, causal):
    """K / V addressed as [seq][head][pos][D] cache rows (what the fused QKV epilogue appends) == the packed-row form, bit
    for bit; cache rows past a sequence's length hold NaN and must never reach the output."""
    lens = [70, 1, 129, 200]
    M, max_len = sum(lens), 256
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    q, k, v = (_rand_bf16(M, H * D, seed=71 + i) for i in range(3))
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    ref = torch.empty(M, H * D, dtype=torch.bfloat16, device=DEV)
    B.attn_fwd(q, k, v, ref, cu_t, max(lens), H, D, D ** -0.5, causal=causal)
    kc = torch.full((len(lens), H, max_len, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    vc = torch.full_like(kc, float("nan"))
    for s, n in enumerate(lens):
        kc[s, :, :n] = k[cu[s]:cu[s + 1]].view(n, H, D).transpose(0, 1)
        vc[s, :, :n] = v[cu[s]:cu[s + 1]].view(n, H, D).transpose(0, 1)
    out = torch.empty_like(ref)
    B.attn_fwd(q, kc, vc, out, cu_t, max(lens), H, D, D ** -0.5, causal=causal, kv_cache_max_len=max_len)
    assert torch.equal(out, ref)


@pytest.mark.parametrize("D,H,causal,bias", [(64, 20, False, False), (64, 12, False, True), (128, 8, True, False), (64, 4, True, False)])
def test_attn_fwd_is_bit_reproducible(B, D, H, causal, bias):
    """The same call five times gives the same bits.  (A row maximum read from an MFMA result before the matrix pipe had
    written it — an instruction-hazard bug of an intermediate round-2 build — showed up only as last-bit differences between
    runs.)  Long enough for many interior tiles, ragged so the masked tail runs too."""
    lens = [1500, 700, 129]
    total = sum(lens)
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    q, k, v = (_rand_bf16(total, H * D, seed=301 + i) for i in range(3))
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    kw = {}
    if bias:
        span = max(lens)
        kw = dict(rel_bias=torch.randn(H, 2 * span - 1, device=DEV), rel_gate=torch.rand(total, H, device=DEV) * 2, rel_span=span)
    outs = []
    for _ in range(5):
        out = torch.empty(total, H * D, dtype=torch.bfloat16, device=DEV)
        B.attn_fwd(q, k, v, out, cu_t, max(lens), H, D, D ** -0.5, causal=causal, **kw)
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0].float()).all()
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


def test_attn_fwd_kv_lens_and_spike(B):
    # key padding + a spiked key that forces the online-softmax rescale late in the sequence
    D, H, lens = 64, 2, [300, 130]
    total = sum(lens)
    cu = [0, 300, 430]
    q, k, v = _rand_bf16(total, H * D, seed=22), _rand_bf16(total, H * D, seed=23), _rand_bf16(total, H * D, seed=24)
    k[250] = (q[10].float() * 4).to(torch.bfloat16)   # huge score for query 10 at key 250 (4th KV tile)
    kv = torch.tensor([260, 100], dtype=torch.int32, device=DEV)
    out = torch.empty(total, H * D, dtype=torch.bfloat16, device=DEV)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    B.attn_fwd(q, k, v, out, cu_t, 300, H, D, 0.125, kv_lens=kv)
    ref = _attn_ref(q, k, v, cu, H, D, 0.125, kv_lens=[260, 100])
    assert (out.float() - ref).abs().max().item() <= 2e-2


def test_attn_fwd_rel_bias(B):
    D, H, lens, span = 64, 4, [333, 90], 333
    total = sum(lens)
    cu = [0, 333, 423]
    q, k, v = _rand_bf16(total, H * D, seed=25), _rand_bf16(total, H * D, seed=26), _rand_bf16(total, H * D, seed=27)
    rel_bias = torch.randn(H, 2 * span - 1, device=DEV)
    rel_gate = torch.rand(total, H, device=DEV) * 2
    out = torch.empty(total, H * D, dtype=torch.bfloat16, device=DEV)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    B.attn_fwd(q, k, v, out, cu_t, 333, H, D, 0.125, rel_bias=rel_bias, rel_gate=rel_gate, rel_span=span)
    ref = _attn_ref(q, k, v, cu, H, D, 0.125, rel_bias=rel_bias, rel_gate=rel_gate, rel_span=span)
    assert (out.float() - ref).abs().max().item() <= 2e-2


@pytest.mark.parametrize("D,H", [(128, 4), (64, 6)])
def test_attn_decode(B, D, H):
    Bn, max_len = 5, 400
    lens = torch.tensor([1, 7, 64, 377, 400], dtype=torch.int32, device=DEV)
    q = _rand_bf16(Bn, H * D, seed=31)
    kc, vc = _rand_bf16(Bn, H, max_len, D, seed=32), _rand_bf16(Bn, H, max_len, D, seed=33)
    out = torch.empty(Bn, H * D, dtype=torch.bfloat16, device=DEV)
    B.attn_decode(q, kc, vc, out, lens, H, D, max_len, D ** -0.5)
    for b in range(Bn):
        L = int(lens[b])
        sc = torch.einsum("hd,hld->hl", q[b].float().view(H, D), kc[b, :, :L].float()) * D ** -0.5
        ref = torch.einsum("hl,hld->hd", torch.softmax(sc, -1), vc[b, :, :L].float()).reshape(-1)
        assert (out[b].float() - ref).abs().max().item() <= 1e-2


@pytest.mark.parametrize("D,H", [(128, 32), (64, 12)])
def test_attn_decode_rounds_the_same_in_any_batch(B, D, H):
    """Few workgroups (a small decode batch) issue 16 key rounds of loads at a time, a full chip 4: the keys of a lane's stream
    and their order are the same, so a (sequence, head) gives bit-identical output alone and among 120 sequences."""
    Bn, max_len = 120, 448
    lens = torch.randint(1, max_len + 1, (Bn,), dtype=torch.int32)
    lens[:4] = torch.tensor([1, 386, 448, 65], dtype=torch.int32)
    lens = lens.to(DEV)
    q = _rand_bf16(Bn, H * D, seed=51)
    kc, vc = _rand_bf16(Bn, H, max_len, D, seed=52), _rand_bf16(Bn, H, max_len, D, seed=53)
    big = torch.empty(Bn, H * D, dtype=torch.bfloat16, device=DEV)
    B.attn_decode(q, kc, vc, big, lens, H, D, max_len, D ** -0.5)          # 120 * H > 1024 workgroups
    for n in (1, 4):
        few = torch.empty(n, H * D, dtype=torch.bfloat16, device=DEV)
        B.attn_decode(q[:n], kc[:n], vc[:n], few, lens[:n], H, D, max_len, D ** -0.5)
        assert torch.equal(few, big[:n])


@pytest.mark.parametrize("D,H,Bn", [(128, 32, 1), (128, 4, 7), (64, 6, 5), (128, 32, 40)])
def test_attn_decode_rope_is_the_two_launches_fused(B, D, H, Bn):
    """icl_attn_decode_rope_bf16 = icl_rope_kv_bf16 (one new position per sequence) + icl_attn_decode_bf16 in ONE launch: the same
    attention output and the same appended cache rows, bit for bit (rope_rot8 and the bf16 rounding of q / k are shared); cache rows
    through a seq_ids indirection; the qkv buffer is left untouched; few and many workgroups."""
    max_len, hd = 448, H * D
    g = torch.Generator().manual_seed(77 + Bn)
    pos = torch.randint(0, max_len - 1, (Bn,), generator=g, dtype=torch.int32)
    pos[0] = 0 if Bn > 1 else 385
    if Bn > 2:
        pos[1], pos[2] = max_len - 1, 63
    lens = (pos + 1).to(DEV)
    pos = pos.to(DEV)
    sid = torch.randperm(Bn, generator=g).to(torch.int32).to(DEV)            # sequence b lives in cache row sid[b]
    qkv = _rand_bf16(Bn, 3 * hd + 64, seed=78)                              # a row stride wider than 3 * hd
    kc, vc = _rand_bf16(Bn, H, max_len, D, seed=79), _rand_bf16(Bn, H, max_len, D, seed=80)
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2, device=DEV).float() / D))
    ang = torch.arange(max_len, device=DEV).float()[:, None] * inv[None, :]
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    # reference: the two launches (rope_kv rotates qkv in place and appends; attention reads cache rows in sequence order)
    qkv_a, kc_a, vc_a = qkv.clone(), kc.clone(), vc.clone()
    B.rope_kv(qkv_a, hd, 2 * hd, cos, sin, pos, sid, kc_a, vc_a, H, D, max_len)
    want = torch.empty(Bn, hd, dtype=torch.bfloat16, device=DEV)
    order = sid.long()
    B.attn_decode(qkv_a[:, :hd], kc_a[order].contiguous(), vc_a[order].contiguous(), want, lens, H, D, max_len, D ** -0.5)
    # fused
    qkv_b, kc_b, vc_b = qkv.clone(), kc.clone(), vc.clone()
    got = torch.empty(Bn, hd, dtype=torch.bfloat16, device=DEV)
    B.attn_decode_rope(qkv_b, hd, 2 * hd, cos, sin, pos, sid, kc_b, vc_b, got, lens, H, D, max_len, D ** -0.5)
    assert torch.equal(got, want)
    assert torch.equal(kc_b, kc_a) and torch.equal(vc_b, vc_a) and torch.equal(qkv_b, qkv)
    for b in range(Bn):                                                      # and the appended rows are where they belong
        assert not torch.equal(kc_b[int(sid[b]), :, int(pos[b])], kc[int(sid[b]), :, int(pos[b])])
    with pytest.raises(B.IclError):
        B.attn_decode_rope(qkv_b, hd, hd, cos, sin, pos, sid, kc_b, vc_b, got, lens, H, D, max_len, D ** -0.5)    # k and v blocks overlap


# ------------------------------------------------------------------------------------------------
# norms / element-wise
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [768, 1280, 2048, 4096, 5120])
@pytest.mark.parametrize("in_dtype", [torch.float32, torch.bfloat16])
def test_layernorm(B, N, in_dtype):
    M = 37
    x = (torch.randn(M, N, device=DEV) * 3 + 1).to(in_dtype)
    g, b = torch.randn(N, device=DEV), torch.randn(N, device=DEV)
    out = torch.empty(M, N, dtype=torch.float32, device=DEV)
    out2 = torch.empty(M, N + 8, dtype=torch.bfloat16, device=DEV)
    B.layernorm(x, g, b, out, 1e-5, out2=out2, N=N)
    ref = torch.nn.functional.layer_norm(x.float(), (N,), g, b, 1e-5)
    assert (out - ref).abs().max().item() <= 2e-5 * ref.abs().max().item() + 1e-5
    assert torch.equal(out2[:, :N], out.to(torch.bfloat16))
    # deep-norm pre-add
    res = torch.randn(M, N, device=DEV).to(in_dtype)
    B.layernorm(x, g, b, out, 1e-5, res=res, alpha=1.7)
    ref = torch.nn.functional.layer_norm(x.float() + 1.7 * res.float(), (N,), g, b, 1e-5)
    assert (out - ref).abs().max().item() <= 2e-5 * ref.abs().max().item() + 1e-5


@pytest.mark.parametrize("N,rms", [(1280, False), (1288, False), (5120, True), (1536, True)])
@pytest.mark.parametrize("in_dtype", [torch.float32, torch.bfloat16])
def test_norm_streaming_variant(B, N, rms, in_dtype):
    """Large activation matrices take the streaming kernel (8-element chunks, persistent waves, next row prefetched): ragged
    row count (not a multiple of the wave grid), strided output, both input dtypes, vs torch and vs the per-row kernel."""
    M = 9001
    x = (torch.randn(M, N, device=DEV) * 2 + 0.5).to(in_dtype)
    g, b = torch.randn(N, device=DEV), torch.randn(N, device=DEV)
    out = torch.empty(M, N + 64, dtype=torch.bfloat16, device=DEV)
    small = torch.empty(64, N + 64, dtype=torch.bfloat16, device=DEV)
    xf = x.float()
    if rms:
        B.rmsnorm(x, g, out, 1e-5, N=N)
        B.rmsnorm(x[:64], g, small, 1e-5, N=N)
        ref = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5) * g
    else:
        B.layernorm(x, g, b, out, 1e-5, N=N)
        B.layernorm(x[:64], g, b, small, 1e-5, N=N)
        ref = torch.nn.functional.layer_norm(xf, (N,), g, b, 1e-5)
    assert _relerr(out[:, :N], ref) < 3e-3
    assert (out[:, :N].float() - ref).abs().max().item() <= 1e-2 * ref.abs().max().item()
    # the kernel choice depends on N and the call form only: a row is bit-identical in any batch
    assert torch.equal(out[:64, :N], small[:, :N])
    f32 = torch.empty(M, N, dtype=torch.float32, device=DEV)
    if rms:
        B.rmsnorm(x, g, f32, 1e-5, N=N)
    else:
        B.layernorm(x, g, b, f32, 1e-5, N=N)
    assert (f32 - ref).abs().max().item() <= 2e-5 * ref.abs().max().item() + 1e-5


@pytest.mark.parametrize("N", [768, 1280, 2048, 4096, 5120])
@pytest.mark.parametrize("rms", [True, False])
def test_norm_few_row_launches_round_like_large_ones(B, N, rms):
    """Launches of few rows (a small decode batch: one to eight rows per call) load gamma / beta ahead of the reductions instead
    of chunk by chunk; the arithmetic is the same, so a row is bit-identical whether it is normalised alone or among 4100."""
    M = 4100
    x = torch.randn(M, N, device=DEV) * 2 + 0.25
    g, b = torch.randn(N, device=DEV), torch.randn(N, device=DEV)
    for dt in (torch.float32, torch.bfloat16):
        big = torch.empty(M, N, dtype=dt, device=DEV)
        for rows in (1, 3, 8):
            few = torch.empty(rows, N, dtype=dt, device=DEV)
            if rms:
                B.rmsnorm(x, g, big, 1e-5)
                B.rmsnorm(x[100:100 + rows], g, few, 1e-5)
            else:
                B.layernorm(x, g, b, big, 1e-5)
                B.layernorm(x[100:100 + rows], g, b, few, 1e-5)
            assert torch.equal(few, big[100:100 + rows]), (N, rms, dt, rows)


@pytest.mark.parametrize("N", [4096, 5120])
def test_rmsnorm(B, N):
    M = 19
    x = torch.randn(M, N, device=DEV) * 2
    g = torch.randn(N, device=DEV)
    out = torch.empty(M, N + 64, dtype=torch.bfloat16, device=DEV)
    B.rmsnorm(x, g, out, 1e-5, N=N)
    ref = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5) * g
    assert torch.equal(out[:, :N], ref.to(torch.bfloat16)) or (out[:, :N].float() - ref).abs().max().item() <= 4e-2
    assert _relerr(out[:, :N], ref) < 3e-3


def test_rope_kv(B):
    H, D, M, max_len, nseq = 4, 128, 11, 32, 3
    qkv = _rand_bf16(M, 3 * H * D, seed=41)
    orig = qkv.clone()
    pos = torch.tensor([0, 1, 2, 3, 0, 1, 5, 6, 7, 30, 31], dtype=torch.int32, device=DEV)
    sid = torch.tensor([0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 2], dtype=torch.int32, device=DEV)
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2, device=DEV).float() / D))
    ang = torch.arange(max_len, device=DEV).float()[:, None] * inv[None, :]
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    kc = torch.zeros(nseq, H, max_len, D, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    B.rope_kv(qkv, H * D, 2 * H * D, cos, sin, pos, sid, kc, vc, H, D, max_len)

    def rot(x):  # x [M, H, D] f32
        c, s = cos[pos.long()][:, None, :], sin[pos.long()][:, None, :]
        x1, x2 = x[..., :D // 2], x[..., D // 2:]
        return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)

    qr = rot(orig[:, :H * D].float().view(M, H, D)).to(torch.bfloat16)
    kr = rot(orig[:, H * D:2 * H * D].float().view(M, H, D)).to(torch.bfloat16)
    assert torch.equal(qkv[:, :H * D].view(M, H, D), qr)
    assert torch.equal(qkv[:, H * D:2 * H * D].view(M, H, D), kr)
    assert torch.equal(qkv[:, 2 * H * D:], orig[:, 2 * H * D:])
    for m in range(M):
        assert torch.equal(kc[sid[m], :, pos[m]], kr[m])
        assert torch.equal(vc[sid[m], :, pos[m]], orig[m, 2 * H * D:].view(H, D))


@pytest.mark.parametrize("M,with_bias", [(600, True), (512, False), (77, True)])
def test_gemm_rope_kv_fused_is_bit_identical(B, M, with_bias):
    """The QKV projection with RoPE + cache append in its epilogue == icl_gemm_bf16 followed by icl_rope_kv_bf16, bit for bit
    (interior tiles, a partial last row of tiles, a single partial tile; with and without the Qwen2 qkv bias)."""
    H, D, K, max_len = 4, 128, 576, 256
    hd = H * D
    x, w = _rand_bf16(M, K, seed=51), _rand_bf16(3 * hd, K, seed=52, scale=0.05)
    bias = torch.randn(3 * hd, device=DEV) if with_bias else None
    lens = [M // 3, M // 3, M - 2 * (M // 3)]
    pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens]).to(DEV)
    sid = torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(lens)]).to(DEV)
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2, device=DEV).float() / D))
    ang = torch.arange(max_len, device=DEV).float()[:, None] * inv[None, :]
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()

    ref = torch.empty(M, 3 * hd, dtype=torch.bfloat16, device=DEV)
    kc0 = torch.zeros(3, H, max_len, D, dtype=torch.bfloat16, device=DEV)
    vc0 = torch.zeros_like(kc0)
    B.gemm(x, w, ref, bias=bias, tile=3)
    B.rope_kv(ref, hd, 2 * hd, cos, sin, pos, sid, kc0, vc0, H, D, max_len)

    out = torch.full((M + 3, 3 * hd), 7.0, dtype=torch.bfloat16, device=DEV)   # 3 guard rows below the matrix
    kc1, vc1 = torch.zeros_like(kc0), torch.zeros_like(kc0)
    B.gemm(x, w, out, bias=bias, tile=3, M=M, rope=(hd, 2 * hd, cos, sin, pos, sid, kc1, vc1, H, D, max_len))
    assert torch.equal(out[:M], ref)
    assert torch.equal(out[M:], torch.full((3, 3 * hd), 7.0, dtype=torch.bfloat16, device=DEV))
    assert torch.equal(kc1, kc0) and torch.equal(vc1, vc0)
    # k / v to the cache only: the q block as before, the k / v column blocks of C untouched
    out3 = torch.full((M, 3 * hd), 7.0, dtype=torch.bfloat16, device=DEV)
    kc2, vc2 = torch.zeros_like(kc0), torch.zeros_like(kc0)
    B.gemm(x, w, out3, bias=bias, tile=3, rope=(hd, 2 * hd, cos, sin, pos, sid, kc2, vc2, H, D, max_len, 0))
    assert torch.equal(out3[:, :hd], ref[:, :hd]) and bool((out3[:, hd:] == 7.0).all())
    assert torch.equal(kc2, kc0) and torch.equal(vc2, vc0)
    with pytest.raises(RuntimeError, match="needs a cache"):
        B.gemm(x, w, out3, bias=bias, tile=3, rope=(hd, 2 * hd, cos, sin, pos, None, None, None, H, D, max_len, 0))
    # and without a cache (training-style forward): rows only
    out2 = torch.empty(M, 3 * hd, dtype=torch.bfloat16, device=DEV)
    B.gemm(x, w, out2, bias=bias, tile=3, rope=(hd, 2 * hd, cos, sin, pos, None, None, None, H, D, max_len))
    assert torch.equal(out2, ref)


def test_gemm_rope_kv_rejects_unfusable(B):
    H, D, K = 3, 128, 256          # 384 columns per block: not a multiple of the 256-column tile
    x, w = _rand_bf16(300, K, seed=53), _rand_bf16(3 * H * D, K, seed=54)
    out = torch.empty(300, 3 * H * D, dtype=torch.bfloat16, device=DEV)
    cs = torch.zeros(8, D // 2, device=DEV)
    pos = torch.zeros(300, dtype=torch.int32, device=DEV)
    assert not B.rope_fusable(300, H, D, K)
    with pytest.raises(RuntimeError, match="icl_gemm_rope_kv_bf16"):
        B.gemm(x, w, out, tile=3, rope=(H * D, 2 * H * D, cs, cs, pos, None, None, None, H, D, 8))


def test_embed_gather_interleave(B):
    V, Hd = 300, 512
    table = _rand_bf16(V, Hd, seed=42)
    speech = torch.randn(20, Hd, device=DEV)
    idx = torch.tensor([5, 299, -1, -20, 0, 17, -3], dtype=torch.int32, device=DEV)
    out = torch.empty(7, Hd, dtype=torch.float32, device=DEV)
    B.embed_gather_interleave(idx, table, speech, out)
    for r, i in enumerate(idx.tolist()):
        ref = table[i].float() if i >= 0 else speech[-i - 1]
        assert torch.equal(out[r], ref)


def test_argmax_eos(B):
    Bn, V = 4, 32001
    logits = torch.randn(Bn, V, device=DEV)
    logits[0, 123] = 50.0
    logits[1, 2] = 50.0            # EOS
    logits[2, 7] = 50.0
    logits[2, 9000] = 50.0         # tie -> lowest index
    logits[3, 32000] = 50.0
    fin = torch.tensor([0, 0, 0, 1], dtype=torch.int32, device=DEV)
    toks = torch.full((Bn, 10), -1, dtype=torch.int32, device=DEV)
    nxt = torch.empty(Bn, dtype=torch.int32, device=DEV)
    B.argmax_eos(logits, 2, 32000, fin, toks, 3, nxt)
    assert toks[:, 3].tolist() == [123, 2, 7, 32000]
    assert nxt.tolist() == [123, 2, 7, 32000]
    assert fin.tolist() == [0, 1, 0, 1]
    assert (toks[:, :3] == -1).all()
    fin2 = torch.zeros(Bn, dtype=torch.int32, device=DEV)       # HF's list form of eos_token_id: either id ends the row
    B.argmax_eos(logits, (2, 7), 32000, fin2, toks, 4, nxt)
    assert toks[:, 4].tolist() == [123, 2, 7, 32000] and fin2.tolist() == [0, 1, 1, 0]


def test_lora_down(B):
    M, K0, r = 9, 4096, 16
    x = _rand_bf16(M, K0 + 64, seed=43)
    x[:, K0:] = 0
    a = _rand_bf16(r, K0, seed=44, scale=0.05)
    ref = (x[:, :K0].float() @ a.float().t() * 2.0)
    B.lora_down(x, K0, a, r, 2.0)
    assert _relerr(x[:, K0:K0 + r], ref) < 4e-3
    assert (x[:, K0 + r:] == 0).all()


@pytest.mark.parametrize("r,K0", [(8, 4096), (16, 1280), (21, 512), (64, 4096), (3, 64)])
def test_lora_down_ranks_and_depths(B, r, K0):
    """rank counts that do not fill the four-row sweeps (3, 21), the maximum (64) and K not a multiple of the 512-wide step"""
    M = 5
    x = _rand_bf16(M, K0 + 64, seed=143)
    x[:, K0:] = 0
    a = _rand_bf16(r, K0, seed=144, scale=0.05)
    ref = (x[:, :K0].float() @ a.float().t() * 0.5)
    B.lora_down(x, K0, a, r, 0.5)
    assert _relerr(x[:, K0:K0 + r], ref) < 4e-3
    assert (x[:, K0 + r:] == 0).all()


def test_beats_patchify_and_posconv_pack_ragged(B):
    """The two BEATs data movers against plain indexing, many ragged audios (every block finds its audio by bisection over
    the packed-row prefix sums): 16x16 patches of the fbank, and the zero-padded per-group image of the positional conv with
    padded rows zeroed in place."""
    rng = np.random.default_rng(7)
    n_audio, max_frames = 37, 160
    frames = rng.integers(1, max_frames // 16 + 1, n_audio) * 16            # whole 16-frame patches
    fb = torch.randn(n_audio, max_frames, 128, device=DEV)
    rows = [int(f // 16) * 8 for f in frames]
    cu = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    total = int(cu[-1])
    out = torch.zeros(total, 256, dtype=torch.bfloat16, device=DEV)
    B.beats_patchify(fb, torch.from_numpy(cu).to(DEV), total, out)
    for a in (0, 1, 17, n_audio - 1):
        T = int(frames[a]) // 16
        ref = fb[a, :T * 16].view(T, 16, 8, 16).permute(0, 2, 1, 3).reshape(T * 8, 256).to(torch.bfloat16)
        assert torch.equal(out[cu[a]:cu[a + 1]], ref), f"patchify: audio {a}"
    # positional-conv image: x [M, C] -> per audio [G][T + 128][C / G] with 64 zero rows in front and behind, padded rows zeroed
    C, G = 768, 16
    T_rows = rng.integers(1, 40, n_audio)
    cu2 = np.concatenate([[0], np.cumsum(T_rows)]).astype(np.int32)
    valid = np.minimum(T_rows, rng.integers(1, 40, n_audio)).astype(np.int32)
    M = int(cu2[-1])
    x = torch.randn(M, C, device=DEV)
    x0 = x.clone()
    xg = torch.full((M + 128 * n_audio, C), float("nan"), dtype=torch.bfloat16, device=DEV).view(-1)
    B.beats_posconv_pack(x, torch.from_numpy(cu2).to(DEV), torch.from_numpy(valid).to(DEV), n_audio, M, G, xg)
    cpg = C // G
    for a in range(n_audio):
        T, v = int(T_rows[a]), int(valid[a])
        xa = x0[cu2[a]:cu2[a + 1]].clone()
        xa[v:] = 0
        assert torch.equal(x[cu2[a]:cu2[a + 1]], xa), f"posconv: audio {a} rows past valid must be zeroed in place"
        img = xg[(int(cu2[a]) + 128 * a) * C:(int(cu2[a + 1]) + 128 * (a + 1)) * C].view(G, T + 128, cpg)
        ref = torch.zeros(G, T + 128, cpg, dtype=torch.bfloat16, device=DEV)
        ref[:, 64:64 + T] = xa.view(T, G, cpg).permute(1, 0, 2).to(torch.bfloat16)
        assert torch.equal(img, ref), f"posconv: audio {a} image"


def test_beats_gate(B):
    M, H = 50, 12
    qkv = _rand_bf16(M, 3 * H * 64, seed=45)
    gw, gb, ga = torch.randn(8, 64, device=DEV) * 0.2, torch.randn(8, device=DEV), torch.rand(H, device=DEV) + 0.5
    gate = torch.empty(M, H, dtype=torch.float32, device=DEV)
    B.beats_gate(qkv, gw, gb, ga, gate, H)
    qh = qkv[:, :H * 64].float().view(M, H, 64)
    proj = (qh @ gw.t() + gb).view(M, H, 2, 4).sum(-1)
    ga_, gb_ = torch.sigmoid(proj[..., 0]), torch.sigmoid(proj[..., 1])
    ref = ga_ * (gb_ * ga[None, :] - 1.0) + 2.0
    assert (gate - ref).abs().max().item() <= 1e-4


def test_qformer_window_xattn(B):
    n_audio, wpa, win, rpa, H = 2, 88, 17, 1500, 12
    q = _rand_bf16(n_audio * wpa, H * 64, seed=46)
    kv = _rand_bf16(n_audio * rpa, 2 * H * 64, seed=47)
    out = torch.empty(n_audio * wpa, H * 64, dtype=torch.bfloat16, device=DEV)
    B.qformer_window_xattn(q, kv, H * 64, out, n_audio, wpa, win, rpa, H, 0.125)
    k = kv[:, :H * 64].float().view(n_audio, rpa, H, 64)[:, :wpa * win].reshape(n_audio * wpa, win, H, 64)
    v = kv[:, H * 64:].float().view(n_audio, rpa, H, 64)[:, :wpa * win].reshape(n_audio * wpa, win, H, 64)
    sc = torch.einsum("whd,wjhd->whj", q.float().view(-1, H, 64), k) * 0.125
    ref = torch.einsum("whj,wjhd->whd", torch.softmax(sc, -1), v).reshape(n_audio * wpa, H * 64)
    assert (out.float() - ref).abs().max().item() <= 1e-2


def test_axpby_cast(B):
    x = torch.randn(13, 70, device=DEV)
    add = _rand_bf16(13, 70, seed=48)
    out = torch.empty(13, 70, dtype=torch.bfloat16, device=DEV)
    B.axpby_cast(x, out, alpha=0.5, add=add)
    assert torch.equal(out, (x * 0.5 + add.float()).to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------
# audio front-ends vs the numpy oracle
# ------------------------------------------------------------------------------------------------
def test_logmel_whisper(B):
    from oracle import audio_frontend as af
    lens = [8000, 116800, 480000]
    wav = torch.zeros(3, 480000, dtype=torch.float32)
    for i, L in enumerate(lens):
        rng = np.random.default_rng(1234 + i)
        wav[i, :L] = torch.from_numpy(np.clip(rng.normal(0, 0.1, L), -1, 1).astype(np.float32))
    wav_d = wav.to(DEV)
    wl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    mel = torch.from_numpy(af.slaney_mel_filters(80)).to(DEV)
    spec = torch.empty(3, 80, 3000, dtype=torch.float32, device=DEV)
    xt = torch.full((3, 3002, 128), float("nan"), dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(3 * 80 * 3000 + 3, dtype=torch.float32, device=DEV)
    B.logmel_whisper(wav_d, wl, mel, 80, spec, xt, ws)
    for i, L in enumerate(lens):
        ref = torch.from_numpy(af.whisper_logmel(wav[i, :L].numpy()))
        err = (spec[i].cpu() - ref).abs().max().item()
        assert err <= 1e-4, (i, err)
    assert (xt[:, 0] == 0).all() and (xt[:, 3001] == 0).all() and (xt[:, :, 80:] == 0).all()
    assert torch.equal(xt[:, 1:3001, :80], spec.transpose(1, 2).to(torch.bfloat16))
    xt2 = torch.empty_like(xt)
    B.spec_to_xt(spec, xt2)
    assert torch.equal(xt, xt2)


def test_fbank_kaldi(B):
    from oracle import audio_frontend as af
    lens = [399 + 160 * 5 + 7, 48000, 480000]
    wav = torch.zeros(3, 480000, dtype=torch.float32)
    for i, L in enumerate(lens):
        rng = np.random.default_rng(77 + i)
        wav[i, :L] = torch.from_numpy(np.clip(rng.normal(0, 0.1, L), -1, 1).astype(np.float32))
    wl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    banks = torch.from_numpy(af.kaldi_mel_banks()).to(DEV)
    max_frames = af.kaldi_num_frames(480000)
    out = torch.full((3, max_frames, 128), float("nan"), dtype=torch.float32, device=DEV)
    B.fbank_kaldi(wav.to(DEV), wl, banks, max_frames, af.FBANK_MEAN, af.FBANK_STD, out)
    for i, L in enumerate(lens):
        ref = torch.from_numpy(af.kaldi_fbank(wav[i, :L].numpy()))
        nf = ref.shape[0]
        assert nf == af.kaldi_num_frames(L)
        err = (out[i, :nf].cpu() - ref).abs().max().item()
        assert err <= 1e-4, (i, err)
        assert torch.isnan(out[i, nf:]).all()


@pytest.mark.parametrize("M", [1, 7, 16, 32, 33, 64])
@pytest.mark.parametrize("N,K", [(4096, 4096), (12288, 4160), (4096, 11008), (1000, 320)])
def test_gemm_skinny_decode_kernel(B, M, N, K):
    a, w = _rand_bf16(M, K, seed=51, scale=0.5), _rand_bf16(N, K, seed=52, scale=0.05)
    bias, res = torch.randn(N, device=DEV), torch.randn(M, N, device=DEV)
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    B.gemm(a, w, out, bias=bias, residual=res, tile=4)
    ref = a.float() @ w.float().t() + bias + res
    assert (out - ref).abs().max().item() <= 2e-3
    out16 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    B.gemm(a, w, out16, tile=4)
    assert _relerr(out16, a.float() @ w.float().t()) < 4e-3


@pytest.mark.parametrize("M,N,K", [(1, 4096, 4096), (8, 1000, 576), (40, 264, 4160), (64, 2048, 64)])
def test_gemm_skinny_on_packed_weights_is_bit_identical(B, M, N, K):
    """tile 6 = the skinny kernel streaming the decode-packed copy: the same MFMAs in the same order as tile 4 on row-major W."""
    a, w = _rand_bf16(M, K, seed=56, scale=0.5), _rand_bf16(N, K, seed=57, scale=0.05)
    bias, res = torch.randn(N, device=DEV), torch.randn(M, N, device=DEV)
    ref = torch.empty(M, N, dtype=torch.float32, device=DEV)
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    B.gemm(a, w, ref, bias=bias, residual=res, tile=4)
    B.gemm(a, B.pack_decode_weights(w), out, bias=bias, residual=res, tile=6, N=N)
    assert torch.equal(out, ref)


@pytest.mark.parametrize("M", [1, 32, 64])
def test_gemm_skinny_swiglu(B, M):
    I, K = 11008 // 4, 512
    a = _rand_bf16(M, K, seed=53, scale=0.5)
    wg, wu = _rand_bf16(I, K, seed=54, scale=0.1), _rand_bf16(I, K, seed=55, scale=0.1)
    w = torch.stack([wg.view(I // 16, 16, K), wu.view(I // 16, 16, K)], dim=1).reshape(2 * I, K).contiguous()
    out = torch.empty(M, I, dtype=torch.bfloat16, device=DEV)
    B.gemm(a, w, out, swiglu=True, tile=4)
    ref = torch.nn.functional.silu(a.float() @ wg.float().t()) * (a.float() @ wu.float().t())
    assert _relerr(out, ref) < 4e-3


@pytest.mark.parametrize("M,N,K,split", [(128, 512, 4160, 1), (128, 4096, 1024, 4), (65, 768, 64, 1), (100, 200, 576, 3),
                                         (97, 12288, 192, 1), (128, 8192, 2048, 5), (77, 264, 320, 5),
                                         (64, 4096, 1024, 2), (9, 520, 576, 1), (33, 1000, 320, 3),     # 64-row blocks
                                         (256, 512, 4160, 1), (200, 4096, 1024, 4), (129, 264, 320, 5), (256, 768, 64, 1)])   # 256-row blocks
def test_gemm_m128_decode_kernel(B, M, N, K, split):
    """Decode tile for M <= 256 (decode-packed weights HBM -> VGPR, activations through an LDS ring): ragged M and N,
    K ranges shorter than the prefetch depth, split-K with uneven slices, f32 + bias + residual and bf16 outputs."""
    a, w = _rand_bf16(M, K, seed=61, scale=0.5), _rand_bf16(N, K, seed=62, scale=0.05)
    bias, res = torch.randn(N, device=DEV), torch.randn(M, N, device=DEV)
    ws = torch.empty(split * M * N, device=DEV) if split > 1 else None
    wp = B.pack_decode_weights(w)
    out = torch.full((M + 2, N), float("nan"), dtype=torch.float32, device=DEV)
    B.gemm(a, wp, out, bias=bias, residual=res, tile=5, split_k=split, workspace=ws, M=M, N=N)
    ref = a.float() @ w.float().t() + bias + res
    assert (out[:M] - ref).abs().max().item() <= 2e-3
    assert torch.isnan(out[M:]).all()
    out16 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    B.gemm(a, wp, out16, tile=5, split_k=split, workspace=ws, N=N)
    assert _relerr(out16, a.float() @ w.float().t()) < 4e-3
    # against the 64x64 tile at the same split: same products, but each slice is summed as (even k-steps) + (odd k-steps)
    out2 = torch.empty(M, N, dtype=torch.float32, device=DEV)
    B.gemm(a, w, out2, bias=bias, residual=res, tile=2, split_k=split, workspace=ws)
    assert (out[:M] - out2).abs().max().item() <= 1e-4


@pytest.mark.parametrize("M,N,K,split,tile", [(256, 4096, 1024, 8, 5), (130, 4096, 2048, 4, 5), (37, 5120, 1024, 2, 5), (256, 4096, 512, 1, 5),
                                              (300, 4096, 1024, 4, 2), (5, 4096, 1024, 1, 6), (5, 4096, 1024, 2, 6), (33, 4096, 1024, 4, 4), (1, 4096, 4096, 1, 6),
                                              (8, 4096, 11008, 1, 6), (40, 4096, 512, 1, 4)])
def test_gemm_rmsnorm_decode_fusion(B, M, N, K, split, tile):
    """icl_gemm_rmsnorm_bf16 (decode: projection back into the residual stream + the RMSNorm that follows, the split-K
    reduction, residual add, row store and normalisation in ONE kernel): the f32 row must be bit-identical to icl_gemm_bf16
    with the same split, the normalised row equal to icl_rmsnorm of it up to the summation order of its sum of squares
    (fixed, but four wave sums instead of one wave per row: <= 1 bf16 ulp on a few elements), in place over the residual.
    split > 1 on the skinny tiles (4 / 6): those kernels split K inside the block and leave no slabs — the entry point must then
    run the plain norm after the GEMM instead of returning with xn unwritten (advisor finding, round 3)."""
    a, w = _rand_bf16(M, K, seed=171, scale=0.5), _rand_bf16(N, K, seed=172, scale=0.05)
    res = torch.randn(M, N, device=DEV)
    gamma = 1.0 + 0.1 * torch.randn(N, device=DEV)
    ws = torch.empty(split * M * N, device=DEV) if split > 1 else None
    wt = B.pack_decode_weights(w) if tile in (5, 6) else w
    h_ref = res.clone()
    B.gemm(a, wt, h_ref, residual=h_ref, tile=tile, split_k=split, workspace=ws, N=N)
    xn_ref = torch.empty(M, N + 64, dtype=torch.bfloat16, device=DEV)
    B.rmsnorm(h_ref, gamma, xn_ref, 1e-5, N=N)
    h = res.clone()
    xn = torch.full((M, N + 64), 7.0, dtype=torch.bfloat16, device=DEV)
    B.gemm_rmsnorm(a, wt, h, gamma, 1e-5, xn, residual=h, tile=tile, split_k=split, workspace=ws, N=N)
    assert torch.equal(h, h_ref)
    assert bool((xn[:, N:] == 7.0).all())                          # the LoRA augmentation columns are not touched
    d = (xn[:, :N].float() - xn_ref[:, :N].float()).abs()
    ulp = xn_ref[:, :N].float().abs() * 2.0 ** -7
    assert bool((d <= ulp + 1e-30).all()) and float((d > 0).float().mean()) < 0.02
    ref = torch.nn.functional.rms_norm(h_ref, (N,), gamma, 1e-5)
    assert _relerr(xn[:, :N], ref) < 4e-3


def test_gemm_m128_rows_do_not_depend_on_the_block_height(B):
    """A row's sums are the same MFMAs in the same order whether it is computed in a 64-, 128- or 256-row block: decoding two
    micro-batches together must not change a sequence's logits."""
    N, K = 1024, 4160
    a, w = _rand_bf16(256, K, seed=161, scale=0.5), _rand_bf16(N, K, seed=162, scale=0.05)
    wp = B.pack_decode_weights(w)
    outs = {}
    for M in (40, 128, 256):
        o = torch.empty(M, N, dtype=torch.float32, device=DEV)
        B.gemm(a[:M], wp, o, tile=5, M=M, N=N)
        outs[M] = o
    assert torch.equal(outs[256][:128], outs[128]) and torch.equal(outs[128][:40], outs[40])


@pytest.mark.parametrize("M,split", [(128, 1), (90, 2), (256, 1), (130, 3)])
def test_gemm_m128_swiglu(B, M, split):
    I, K = 11008 // 4, 512
    a = _rand_bf16(M, K, seed=63, scale=0.5)
    wg, wu = _rand_bf16(I, K, seed=64, scale=0.1), _rand_bf16(I, K, seed=65, scale=0.1)
    w = torch.stack([wg.view(I // 16, 16, K), wu.view(I // 16, 16, K)], dim=1).reshape(2 * I, K).contiguous()
    ws = torch.empty(split * M * 2 * I, device=DEV) if split > 1 else None
    out = torch.empty(M, I, dtype=torch.bfloat16, device=DEV)
    B.gemm(a, B.pack_decode_weights(w), out, swiglu=True, tile=5, split_k=split, workspace=ws, N=2 * I)
    ref = torch.nn.functional.silu(a.float() @ wg.float().t()) * (a.float() @ wu.float().t())
    assert _relerr(out, ref) < 4e-3


def _sample_case(logits, prev, step, temp, k, p, pen, u, eos=-1, pad=0, finished=None):
    from icl_speech_text_llm_amd.runtime import binding as Bd
    Bn, V = logits.shape
    dev = "cuda"
    lg = logits.to(dev).contiguous()
    toks = torch.zeros(Bn, 16, dtype=torch.int32, device=dev)
    if step:
        toks[:, :step] = prev[:, :step].to(torch.int32).to(dev)
    fin = torch.zeros(Bn, dtype=torch.int32, device=dev) if finished is None else finished.to(torch.int32).to(dev)
    nxt = torch.zeros(Bn, dtype=torch.int32, device=dev)
    work = torch.empty(Bn, V, dtype=torch.float32, device=dev)
    dbg = (torch.full((Bn, 1024), -1, dtype=torch.int32, device=dev), torch.zeros(Bn, 1024, device=dev),
           torch.zeros(Bn, dtype=torch.int32, device=dev))
    Bd.sample_eos(lg, work, u.to(dev), eos, pad, fin, toks, step, nxt, temperature=temp, top_k=k, top_p=p,
                  repetition_penalty=pen, debug=dbg)
    torch.cuda.synchronize()
    return toks.cpu(), nxt.cpu(), fin.cpu(), [d.cpu() for d in dbg]


def test_sample_eos_matches_oracle_and_hf_golden():
    """Sampled decode tail (csrc/sampling.hip) vs the oracle's restatement of HF's logits processors: kept tokens in draw order
    (exact), probabilities (1e-6), the inverse-CDF pick for given uniforms (exact away from CDF boundaries), ties at the
    top-k boundary, repetition penalty on tokens inside the nucleus, full Llama (32001) and Qwen (156032) vocabularies."""
    import os
    from oracle import models as om
    g = torch.Generator().manual_seed(5)
    for V, temp, k, p, pen in ((32001, 0.8, 50, 0.9, 1.0), (32001, 0.8, 50, 0.9, 1.3), (156032, 0.7, 20, 0.5, 1.1),
                               (777, 1.0, 5, 0.5, 1.0), (260, 1.5, 200, 0.99, 1.2), (32001, 1.0, 1000, 1.0, 1.0),
                               (32001, 0.6, 1, 1.0, 1.5)):
        Bn, step = 5, 6
        logits = torch.randn(Bn, V, generator=g) * 3.0
        logits[1, 100:110] = logits[1].max() + 0.25
        prev = torch.randint(0, V, (Bn, 16), generator=g)
        prev[2, :3] = logits[2].topk(3).indices
        u = torch.rand(Bn, generator=g)
        toks, nxt, fin, (ids, probs, cnt) = _sample_case(logits, prev, step, temp, k, p, pen, u)
        for b in range(Bn):
            oi, op = om.sample_filter(logits[b].numpy(), prev[b, :step].tolist(), pen, temp, k, p)
            n = int(cnt[b])
            assert n == len(oi), (V, b, n, len(oi))
            assert ids[b, :n].tolist() == oi.tolist(), (V, b)
            assert float((probs[b, :n] - torch.from_numpy(op)).abs().max()) < 1e-6, (V, b)
            cdf = np.cumsum(op.astype(np.float64))
            if np.abs(cdf - float(u[b])).min() > 1e-5:
                assert int(nxt[b]) == int(oi[om.sample_pick(op, float(u[b]))]), (V, b)
            assert int(toks[b, step]) == int(nxt[b]) and toks[b, :step].tolist() == prev[b, :step].tolist()
    # the HF golden (tests/golden/sampling.npz) through the kernel
    a = np.load(os.path.join(os.path.dirname(__file__), "golden", "sampling.npz"))
    for i in range(7):
        temp, k, p, pen = a[f"knobs_{i}"].tolist()
        logits, prev = torch.from_numpy(a[f"logits_{i}"]), torch.from_numpy(a[f"prev_{i}"])
        prev16 = torch.zeros(3, 16, dtype=torch.long)
        prev16[:, :6] = prev
        _, _, _, (ids, probs, cnt) = _sample_case(logits, prev16, 6, temp, int(k), p, pen, torch.rand(3, generator=g))
        for b in range(3):
            want = a[f"probs_{i}"][b]
            kept = np.nonzero(want > 0)[0]
            n = int(cnt[b])
            assert n == len(kept), (i, b)
            assert np.abs(np.sort(probs[b, :n].numpy()) - np.sort(want[kept])).max() < 2e-6, (i, b)
    # bookkeeping: a finished row emits pad whatever the draw; a drawn EOS finishes the row
    logits = torch.randn(2, 300, generator=g)
    top = int(logits[1].argmax())
    toks, nxt, fin, _ = _sample_case(logits, torch.zeros(2, 16, dtype=torch.long), 0, 1.0, 1, 1.0, 1.0, torch.zeros(2),
                                     eos=top, pad=7, finished=torch.tensor([1, 0]))
    assert nxt.tolist() == [7, top] and fin.tolist() == [1, 1]


def test_sample_eos_without_top_k_normalises_over_the_whole_row():
    """top_k == V = HF's "top-k off" (top_k 0 / None; TopKLogitsWarper clamps to the vocabulary): the kept set and its
    probabilities must be HF's top-p over the WHOLE distribution whenever the nucleus fits the kernel's 1024-entry candidate
    list; a small vocabulary fits whatever top_p is (incl. 1.0 = the full softmax)."""
    from oracle import models as om
    g = torch.Generator().manual_seed(11)
    for V, temp, p, pen, scale in ((777, 1.0, 1.0, 1.0, 2.0), (777, 0.7, 0.6, 1.2, 2.0), (32001, 0.8, 0.9, 1.0, 6.0), (156032, 0.7, 0.5, 1.1, 8.0)):
        Bn, step = 4, 5
        logits = torch.randn(Bn, V, generator=g) * scale
        prev = torch.randint(0, V, (Bn, 16), generator=g)
        u = torch.rand(Bn, generator=g)
        toks, nxt, fin, (ids, probs, cnt) = _sample_case(logits, prev, step, temp, V, p, pen, u)
        for b in range(Bn):
            oi, op = om.sample_filter(logits[b].numpy(), prev[b, :step].tolist(), pen, temp, V, p)
            assert len(oi) <= 1000, "test case must keep the nucleus inside the candidate list"
            n = int(cnt[b])
            assert abs(n - len(oi)) <= 1, (V, b, n, len(oi))          # the cut sums the mass from the other end than HF does
            m = min(n, len(oi))
            assert ids[b, :m].tolist() == oi[:m].tolist(), (V, b)
            if n == len(oi):
                assert float((probs[b, :n] - torch.from_numpy(op)).abs().max()) < 2e-6, (V, b)
            assert int(nxt[b]) in ids[b, :n].tolist()
    with pytest.raises(Exception):                                    # between the candidate-list size and V: an argument error
        _sample_case(torch.randn(1, 32001), torch.zeros(1, 16, dtype=torch.long), 0, 1.0, 2000, 0.9, 1.0, torch.zeros(1))


# ---- beam search: the step kernel against the oracle's scorer, the span copy against indexing -----------------------------------
@pytest.mark.parametrize("Bn,K,V,T,lp,eos", [(3, 4, 260, 6, 1.0, 17), (2, 8, 32001, 5, 2.0, 2), (5, 1, 40, 4, 0.0, 3),
                                              (2, 3, 1000, 64, -1.0, 5), (1, 2, 4, 3, 1.0, 0), (3, 4, 300, 6, 1.0, (17, 40)),
                                              (2, 8, 32001, 4, -1.0, (2, 31999)), (2, 2, 6, 3, 1.0, (0, 5))])
@pytest.mark.parametrize("pen", [1.0, 1.6])
def test_beam_step_matches_oracle_scorer(B, Bn, K, V, T, lp, eos, pen):
    """Scores: f32 log-softmax over up to 32001 columns summed in another order than torch (2e-5 relative).
    A whole search on synthetic logits that depend on each beam's history (a tiny recurrent stand-in for the decoder, advanced
    along the chosen parents): `icl_beam_step` and oracle.BeamBookkeeping must choose the same parents / tokens at every step and
    return the same hypotheses; peaked columns make EOS and a few exact ties (lower beam*V + token wins) part of the race."""
    from oracle import models as om
    g = torch.Generator().manual_seed(Bn * 1000 + K * 10 + T)
    Hd = 12
    A = torch.randn(Hd, Hd, generator=g) * 0.6
    E = torch.randn(V, Hd, generator=g)
    U = torch.randn(Hd, V, generator=g) * 1.5
    U[:, list(eos) if isinstance(eos, tuple) else eos] += 0.8     # EOS is a frequent contender (a tuple: HF's list of EOS ids, 3K kept)
    h = torch.randn(Bn, Hd, generator=g)
    state = B.BeamState(lambda name, shape, dt: torch.empty(shape, dtype=dt, device=DEV), Bn, K, T, pad_id=V - 1)
    bk = om.BeamBookkeeping(Bn, K, T, eos, lp, pen)

    def logits_of(hid):
        lg = (hid @ U).float()
        if V > 20:
            lg[:, 7] = lg[:, 11]                        # an exact tie between two tokens of every beam
        return lg.contiguous()
    hid = h
    lg = logits_of(hid)                                 # step 0: one distribution per row
    for s in range(T):
        B.beam_step(lg.to(DEV), state, s, eos, lp, repetition_penalty=pen)
        lg_bk = lg if lg.shape[0] == Bn * K else lg.repeat_interleave(K, 0)
        was_open = list(bk.open)
        parents, toks = bk.step(lg_bk)
        gp, gt = state.parent.cpu().long(), state.next_ids.cpu().long()
        if s + 1 < T:
            assert torch.equal(gt, toks) and torch.equal(gp, parents), (s, gt, toks, gp, parents)
        fin_s = torch.stack([torch.stack([f[0] for f in bk.fin[b]]) for b in range(Bn)])
        assert torch.allclose(state.fin_score.cpu(), fin_s, rtol=2e-5, atol=2e-5), (s, state.fin_score.cpu(), fin_s)
        assert state.unsat.cpu().tolist() == [int(o) for o in bk.open], (s, was_open)
        for b in range(Bn):
            for k in range(K):
                if bk.fin[b][k][2]:
                    n = len(bk.fin[b][k][1])
                    assert int(state.fin_len[b, k]) == n and state.fin_seq[b, k, :n].cpu().tolist() == bk.fin[b][k][1]
        if s + 1 == T:
            break
        hid_rows = hid if hid.shape[0] == Bn * K else hid.repeat_interleave(K, 0)
        hid = torch.tanh(hid_rows[parents] @ A + E[toks])
        lg = logits_of(hid)
    want, score = bk.result(V - 1)
    n = state.fin_len[:, 0].cpu()
    for b in range(Bn):
        assert state.fin_seq[b, 0, :int(n[b])].cpu().tolist() == [t for t in want[b].tolist()][:int(n[b])]
    assert torch.allclose(state.fin_score[:, 0].cpu(), score, rtol=2e-5, atol=2e-5)


def test_beam_step_with_nan_logits_keeps_parents_inside_the_row(B):
    """A NaN logit is a token that cannot be chosen (as in icl_argmax_eos); a row of nothing but NaN still yields parents inside
    [b*K, b*K+K) and tokens inside [0, V) — `parent` feeds icl_kv_copy_spans_bf16 as a sequence id (advisor finding, round 3)."""
    Bn, K, V, T = 3, 4, 500, 4
    st = B.BeamState(lambda name, shape, dt: torch.empty(shape, dtype=dt, device=DEV), Bn, K, T, pad_id=0)
    g = torch.Generator().manual_seed(3)
    lg = torch.randn(Bn, V, generator=g)
    lg[0, 17] = float("nan")                    # one NaN among good logits
    lg[1, :] = float("nan")                     # a whole row of NaN
    B.beam_step(lg.to(DEV), st, 0, 2, 1.0)
    for step in (1, 2):
        lgk = torch.randn(Bn * K, V, generator=g)
        lgk[0:K, 33] = float("nan")
        lgk[K + 1, :] = float("nan")            # one beam of row 1 is all NaN
        lgk[2 * K:3 * K, :] = float("nan")      # every beam of row 2
        B.beam_step(lgk.to(DEV), st, step, 2, 1.0)
        par, nxt = st.parent.cpu().view(Bn, K), st.next_ids.cpu().view(Bn, K)
        for b in range(Bn):
            assert bool(((par[b] >= b * K) & (par[b] < b * K + K)).all()), (step, b, par[b])
            assert bool(((nxt[b] >= 0) & (nxt[b] < V)).all()), (step, b, nxt[b])
        assert 33 not in nxt[0].tolist()
    assert 17 not in st.run_seq.cpu()[0, :, 0].tolist()
    # the same first step with the NaN replaced by a hopeless finite logit: row 0's choices are the same
    st2 = B.BeamState(lambda name, shape, dt: torch.empty(shape, dtype=dt, device=DEV), Bn, K, T, pad_id=0)
    lg2 = lg.clone()
    lg2[0, 17] = -1e30
    st3 = B.BeamState(lambda name, shape, dt: torch.empty(shape, dtype=dt, device=DEV), Bn, K, T, pad_id=0)
    B.beam_step(lg2.to(DEV), st2, 0, 2, 1.0)
    B.beam_step(lg.to(DEV), st3, 0, 2, 1.0)
    assert torch.equal(st2.next_ids.cpu()[:K], st3.next_ids.cpu()[:K])


def test_kv_copy_spans_clamps_corrupt_ids(B):
    """Sequence ids / starts / counts read from device memory are clamped to the extents the caller described (ABI 5)."""
    L, S, H, P, D = 2, 4, 2, 8, 64
    src = torch.randn(L, S, H, P, D, device=DEV).to(torch.bfloat16)
    dst = torch.zeros(L, S, H, P, D, dtype=torch.bfloat16, device=DEV)
    guard = torch.zeros(1 << 16, dtype=torch.bfloat16, device=DEV)      # noqa: F841 (keeps a neighbour allocation alive)
    bad = torch.tensor([0x7fffffff // 500, -5, 2, 3], dtype=torch.int32, device=DEV)
    n_t = torch.tensor([3, 100, 2, -1], dtype=torch.int32, device=DEV)
    B.kv_copy_spans(src, dst, 4, src_seq=bad, n_t=n_t)
    torch.cuda.synchronize()
    assert torch.equal(dst[:, 0, :, :3], src[:, S - 1, :, :3])          # id clamped to the last sequence
    assert torch.equal(dst[:, 1], src[:, 0])                            # id clamped to 0, count clamped to the 8 positions
    assert torch.equal(dst[:, 2, :, :2], src[:, 2, :, :2]) and not bool(dst[:, 3].any())


def test_beam_step_rejects_bad_arguments(B):
    st = B.BeamState(lambda name, shape, dt: torch.empty(shape, dtype=dt, device=DEV), 2, 2, 4, pad_id=0)
    lg = torch.zeros(2, 3, device=DEV)
    with pytest.raises(B.IclError):
        B.beam_step(lg, st, 0, 1, 1.0)                  # V < 2 * num_beams
    with pytest.raises(B.IclError):
        B.beam_step(torch.zeros(2, 50, device=DEV), st, 4, 1, 1.0)      # step outside [0, T)
    st9 = B.BeamState(lambda name, shape, dt: torch.empty(shape, dtype=dt, device=DEV), 1, 9, 4, pad_id=0)
    with pytest.raises(B.IclError):
        B.beam_step(torch.zeros(1, 50, device=DEV), st9, 0, 1, 1.0)     # more than 8 beams


def test_kv_copy_spans(B):
    """Prompt rows to the beams of a row (ragged lengths), then generated positions from each beam's parent via a staging buffer."""
    L, S, H, P, D = 3, 8, 2, 24, 64
    cache = torch.randn(L, S, H, P, D, device=DEV).to(torch.bfloat16)
    ref = cache.clone()
    view, rview = cache[:, :6], ref[:, :6]             # six beam sequences + two prompt rows: a view with the parent's strides
    src = torch.tensor([6, 6, 6, 7, 7, 7], dtype=torch.int32, device=DEV)
    n_t = torch.tensor([5, 5, 5, 9, 9, 0], dtype=torch.int32, device=DEV)
    B.kv_copy_spans(cache, cache, 6, src_seq=src, n_t=n_t)
    for r in range(6):
        n = int(n_t[r])
        ref[:, r, :, :n] = ref[:, int(src[r]), :, :n]
    assert torch.equal(cache, ref)
    parent = torch.tensor([1, 0, 0, 5, 3, 4], dtype=torch.int32, device=DEV)
    t0 = torch.tensor([5, 5, 5, 9, 9, 9], dtype=torch.int32, device=DEV)
    tmp = torch.zeros(L, 6, H, 4, D, dtype=torch.bfloat16, device=DEV)
    B.kv_copy_spans(view, tmp, 6, src_seq=parent, src_t0=t0, n_fixed=3)
    B.kv_copy_spans(tmp, view, 6, dst_t0=t0, n_fixed=3)
    want = rview.clone()
    for r in range(6):
        a = int(t0[r])
        want[:, r, :, a:a + 3] = rview[:, int(parent[r]), :, a:a + 3]
    assert torch.equal(view, want) and torch.equal(cache[:, 6:], ref[:, 6:])
    assert torch.equal(tmp[:, :, :, 3], torch.zeros_like(tmp[:, :, :, 3]))
    B.kv_copy_spans(view, tmp, 6, n_fixed=0)           # nothing to copy: no launch, no error
    with pytest.raises(B.IclError):
        B.kv_copy_spans(cache.cpu(), tmp, 6, n_fixed=1)

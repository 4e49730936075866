"""Every GEMM launch a decode step plans (runtime/engines.py: decode_plan), issued as the plan says on one layer of real-size
weights packed by LlamaHIP, against a float64 torch reference of the same operation with per-element bounds (`-m gpu`).

Models: Llama-2-7B (LoRA-augmented QKV K), Llama-2-13B, Qwen2-Audio's Qwen2-7B decoder (QKV bias, vocab 156032).  Batches at
every point where the plan changes kernel or split.  Weight modes: bf16 on the decode-packed copies (the default), bf16 without
them, FP8 weights (reference on W'), and bf16 with every site kept on the decode tile above 128 rows (ICL_DECODE_T256="").
Every output element is checked (outputs start as NaN: a tile the grid misses fails), and the split-K workspace is followed by
a NaN guard that must survive.

Bounds (u = 2^-24, C_DOT = 2; |a| @ |W|^T taken in float64):
- f32 C:      |C - ref| <= C_DOT * K * u * (|a| @ |W|^T) + u * |ref| + 2u * (|bias| + |residual|)
- bf16 out:   the f32 bound + 1 bf16 ulp of max(|ref|, |out|)
- SwiGLU act: the f32 bounds of gate and up propagated through silu(g) * u (|silu'| <= 1.1), silu's own f32 error
              (fast exp / rcp: u * (16 + 4 |g|) relative) + 1 bf16 ulp
- xn:         1 bf16 ulp of the float64 RMSNorm of the kernel's own C row

Also the gemm_rmsnorm split_k == 1 contract (include/icl_hip.h): C bit-identical to icl_gemm_bf16, -0.0 included; xn within
1 bf16 ulp of icl_rmsnorm of that C (bit-identical where the header says icl_rmsnorm runs)."""
import dataclasses

import pytest
import torch

from fp64_bounds import C_DOT, U, _dot, assert_within, bf16_ulp
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

GUARD = 4096
BATCHES = (1, 8, 9, 64, 65, 128, 129, 255, 256, 257)
MODELS = ("llama2_7b", "llama2_13b", "qwen2_7b")
MODES = ("bf16", "bf16_row_major", "fp8")


def _cfg(model):
    from icl_speech_text_llm_amd.runtime.config import QwenAudioCfg, SalmonnCfg
    return {"llama2_7b": SalmonnCfg.llama2_7b().llama, "llama2_13b": SalmonnCfg.llama2_13b().llama,
            "qwen2_7b": QwenAudioCfg().llm}[model]


_RT = {}


def _runtimes(model):
    """(bf16 LlamaHIP, fp8 LlamaHIP) over one decoder layer of seeded real-size weights; one model is kept at a time."""
    if model not in _RT:
        _RT.clear()
        _W64.clear()
        torch.cuda.empty_cache()
        from icl_speech_text_llm_amd.runtime import synth
        from icl_speech_text_llm_amd.runtime.engines import LlamaHIP
        from icl_speech_text_llm_amd.runtime.packing import pack_llama
        cfg = dataclasses.replace(_cfg(model), n_layers=1)
        sd = synth.llama_state(cfg, synth._Gen(7, DEV, torch.bfloat16, jitter=True))
        out = []
        for wd in ("bf16", "fp8"):
            rt = LlamaHIP(pack_llama(sd, cfg, DEV), DEV, decode_packed=True, weight_dtype=wd)
            L = rt.w.layers[0]
            if L.bqkv is not None:   # a bias well above the GEMM's error bound, so a bias the kernel drops is seen
                L.bqkv = torch.randn(L.bqkv.shape, generator=torch.Generator(DEV).manual_seed(3), device=DEV)
            out.append(rt)
        del sd
        _RT[model] = tuple(out)
    return _RT[model]


def _rand(shape, seed, dtype=torch.bfloat16):
    g = torch.Generator(DEV).manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV).to(dtype)


def _rms64(c, gamma, eps):
    c = c.double()
    return c * torch.rsqrt(c.pow(2).mean(-1, keepdim=True) + eps) * gamma.double()


_W64 = {}


def _w64(t):
    key = (t.data_ptr(), tuple(t.shape))
    if key not in _W64:
        if len(_W64) > 12:
            _W64.clear()
        w = t.double()
        _W64[key] = (w, w.abs())
    return _W64[key]


def _case_list():
    cases = [(m, bn, mode) for m in MODELS for mode in MODES for bn in BATCHES]
    cases += [(m, bn, "bf16_decode_tile") for m in MODELS for bn in (129, 255, 256)]
    return cases


@pytest.mark.parametrize("model,Bn,mode", _case_list())
def test_decode_step_gemm_launches_against_fp64(B, model, Bn, mode):
    from icl_speech_text_llm_amd.runtime import engines as E
    rt16, rt8 = _runtimes(model)
    rt = rt8 if mode == "fp8" else rt16
    c, L = rt.w.cfg, rt.w.layers[0]
    hd, I, ka = c.hidden, c.ffn, rt.w.k_aug
    plan = E.decode_plan(Bn, c, ka, rt.n_cu, rt.weight_dtype, mode != "bf16_row_major",
                         () if mode == "bf16_decode_tile" else rt.decode_t256)
    if mode in ("bf16", "fp8"):
        assert plan == rt.decode_plan(Bn)          # the runtime's own plan
    if any(p.weight == "packed" for p in plan.sites.values()):
        rt.ensure_decode_packed()
    forms = {"qkv": (0, L.wqkv), "o": (1, L.wo), "gu": (2, L.wgu), "down": (3, L.wdown)}

    def weight(name):
        idx, row = forms[name]
        p = plan.sites[name]
        if p.weight == "fp8":
            return L.fp8[idx][0], L.fp8[idx][1]
        return (L.decode_packed[idx] if p.weight == "packed" else row), None

    ws_all = torch.full((plan.workspace + GUARD,), float("nan"), device=DEV)
    wsk = ws_all[:plan.workspace] if plan.workspace else None
    launched = []

    # ---- qkv: bf16 out = xn_aug @ Wqkv^T (+ the Qwen2 bias) ----------------------------------------------------------
    p = plan.sites["qkv"]
    xn = _rand((Bn, ka), 11)
    qkv = torch.full((Bn, 3 * hd), float("nan"), dtype=torch.bfloat16, device=DEV)
    w, s = weight("qkv")
    B.gemm(xn, w, qkv, bias=L.bqkv, split_k=p.split_k, workspace=wsk, tile=p.tile, N=3 * hd, K=ka, w_scale=s)
    launched.append(("qkv", p))
    ref, mag = _dot(xn, *_w64(L.wqkv))
    b = L.bqkv.double() if L.bqkv is not None else torch.zeros(3 * hd, dtype=torch.float64, device=DEV)
    ref = ref + b
    e = C_DOT * ka * U * mag + U * ref.abs() + 2 * U * b.abs()
    assert_within(qkv, ref, e + bf16_ulp(torch.maximum(ref.abs(), qkv.double().abs())), f"qkv {p}")

    # ---- o: h += att @ Wo^T in place (f32), xn = rmsnorm(h) * rms2 (fused) --------------------------------------------
    p = plan.sites["o"]
    att = _rand((Bn, hd), 12)
    h = _rand((Bn, hd), 13, torch.float32)
    h0 = h.clone()
    xo = torch.full((Bn, ka), float("nan"), dtype=torch.bfloat16, device=DEV)
    xo[:, hd:] = 7.0                                   # the LoRA tail of the layer's xn buffer must survive
    w, s = weight("o")
    assert p.fused_norm
    B.gemm_rmsnorm(att, w, h, L.rms2, c.rms_eps, xo, residual=h, split_k=p.split_k, workspace=wsk, tile=p.tile, N=hd, K=hd,
                   w_scale=s)
    launched.append(("o", p))
    ref, mag = _dot(att, *_w64(L.wo))
    ref = ref + h0.double()
    assert_within(h, ref, C_DOT * hd * U * mag + U * ref.abs() + 2 * U * h0.double().abs(), f"o C {p}")
    xr = _rms64(h, L.rms2, c.rms_eps)
    assert_within(xo[:, :hd], xr, bf16_ulp(torch.maximum(xr.abs(), xo[:, :hd].double().abs())), f"o xn {p}")
    assert bool((xo[:, hd:] == 7.0).all()), "o: xn written past N"

    # ---- gu: act = silu(gate) * up, gate / up interleaved in blocks of 16 rows (bf16 out) ---------------------------------
    p = plan.sites["gu"]
    xg = _rand((Bn, hd), 14)
    act = torch.full((Bn, I), float("nan"), dtype=torch.bfloat16, device=DEV)
    w, s = weight("gu")
    B.gemm(xg, w, act, swiglu=True, K=hd, split_k=p.split_k, workspace=wsk, tile=p.tile, N=2 * I, w_scale=s)
    launched.append(("gu", p))
    w64, w64a = _w64(L.wgu)
    gate, gmag = _dot(xg, w64.view(I // 16, 2, 16, hd)[:, 0].reshape(I, hd), w64a.view(I // 16, 2, 16, hd)[:, 0].reshape(I, hd))
    up, umag = _dot(xg, w64.view(I // 16, 2, 16, hd)[:, 1].reshape(I, hd), w64a.view(I // 16, 2, 16, hd)[:, 1].reshape(I, hd))
    sg = gate * torch.sigmoid(gate)
    ref = sg * up
    eg = C_DOT * hd * U * gmag + U * gate.abs()
    eu = C_DOT * hd * U * umag + U * up.abs()
    e = 1.1 * eg * (up.abs() + eu) + sg.abs() * eu + U * (16 + 4 * gate.abs()) * ref.abs()
    assert_within(act, ref, e + bf16_ulp(torch.maximum(ref.abs(), act.double().abs())), f"gu {p}")

    # ---- down: h += act @ Wdown^T in place (f32), xn = rmsnorm(h) * the next norm's gamma (fused) ------------------------
    p = plan.sites["down"]
    a_in = _rand((Bn, I), 15)
    h = _rand((Bn, hd), 16, torch.float32)
    h0 = h.clone()
    xd = torch.full((Bn, hd), float("nan"), dtype=torch.bfloat16, device=DEV)
    w, s = weight("down")
    assert p.fused_norm
    B.gemm_rmsnorm(a_in, w, h, rt.w.norm, c.rms_eps, xd, residual=h, split_k=p.split_k, workspace=wsk, tile=p.tile, N=hd, K=I,
                   w_scale=s)
    launched.append(("down", p))
    ref, mag = _dot(a_in, *_w64(L.wdown))
    ref = ref + h0.double()
    assert_within(h, ref, C_DOT * I * U * mag + U * ref.abs() + 2 * U * h0.double().abs(), f"down C {p}")
    xr = _rms64(h, rt.w.norm, c.rms_eps)
    assert_within(xd, xr, bf16_ulp(torch.maximum(xr.abs(), xd.double().abs())), f"down xn {p}")

    torch.cuda.synchronize()
    assert bool(torch.isnan(ws_all[plan.workspace:]).all()), "a split-K launch wrote past the planned workspace"
    assert {n for n, _ in launched} == set(E.DECODE_SITES)


@pytest.mark.parametrize("model", MODELS)
def test_lm_head_launch_against_fp64(B, model):
    """The LM head as logits() issues it (tile 4 at <= 8 rows, the library's choice above) over every logit of an odd vocab
    (32001 / 156032), at the rows where the choice changes and at a ragged M edge."""
    from icl_speech_text_llm_amd.runtime import engines as E
    rt = _runtimes(model)[0]
    c = rt.w.cfg
    w64 = _w64(rt.w.lm_head)
    for R in (1, 8, 9, 65, 257):
        p = E.decode_plan(R, c, rt.w.k_aug, rt.n_cu).sites["lm_head"]
        assert p.tile == E.lm_head_tile(R) and (p.N, p.K) == (c.vocab, c.hidden)
        xf = _rand((R, c.hidden), 21)
        out = torch.full((R, c.vocab), float("nan"), device=DEV)
        B.gemm(xf, rt.w.lm_head, out, tile=p.tile)
        ref, mag = _dot(xf, *w64)
        assert_within(out, ref, C_DOT * c.hidden * U * mag + U * ref.abs(), f"lm_head R={R} {p}")
        # logits() itself: the final norm, then the same launch
        h = _rand((R, c.hidden), 22, torch.float32)
        ws = E.Workspace(DEV)
        got = rt.logits(ws, h, name="t_logits")
        xn = ws.get("t_logits_xn", (R, c.hidden), torch.bfloat16)
        ref, mag = _dot(xn, *w64)
        assert_within(got, ref, C_DOT * c.hidden * U * mag + U * ref.abs(), f"logits() R={R}")
    _W64.clear()


# ---- icl_gemm_rmsnorm_bf16 with split_k == 1 --------------------------------------------------------------------------
@pytest.mark.parametrize("tile", (2, 4, 6))
@pytest.mark.parametrize("M", (1, 8, 64, 65))
@pytest.mark.parametrize("wide", (False, True))
def test_gemm_rmsnorm_split1_contract(B, tile, M, wide):
    """C bit-identical to icl_gemm_bf16 with the same arguments (compared as int32, so -0.0 != +0.0); xn within 1 bf16 ulp of
    icl_rmsnorm of that C, and bit-identical to it where include/icl_hip.h says icl_rmsnorm runs (M > 64 or ldc != N).  Rows 0
    and M - 1 have zero activations and a -0.0 residual."""
    if tile in (4, 6) and M > 64:
        pytest.skip("the skinny kernels take M <= 64")
    N = K = 4096
    w = _rand((N, K), 31) * 0.02
    wk = B.pack_decode_weights(w) if tile == 6 else w
    a = _rand((M, K), 32)
    a[0] = 0
    a[M - 1] = 0
    res = _rand((M, N), 33, torch.float32)
    res[0] = -0.0
    res[M - 1] = -0.0
    gamma = 1 + 0.1 * _rand((N,), 34, torch.float32)
    eps = 1e-5
    ld = N + 64 if wide else N

    def buf():
        t = torch.full((M, ld), float("nan"), device=DEV)[:, :N]
        t.copy_(res)
        return t
    c1, c2 = buf(), buf()
    x1 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    x2 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    B.gemm_rmsnorm(a, wk, c1, gamma, eps, x1, residual=c1, split_k=1, tile=tile, N=N, K=K)
    B.gemm(a, wk, c2, residual=c2, split_k=1, tile=tile, N=N, K=K)
    B.rmsnorm(c2, gamma, x2, eps)
    torch.cuda.synchronize()
    neg0 = int(((c2 == 0) & torch.signbit(c2)).sum())
    print(f"tile {tile} M {M} ldc {ld}: {neg0} -0.0 in icl_gemm_bf16's C")
    assert torch.equal(c1.contiguous().view(torch.int32), c2.contiguous().view(torch.int32))
    if M > 64 or wide:
        assert torch.equal(x1.view(torch.int16), x2.view(torch.int16))
    d = (x1.double() - x2.double()).abs()
    assert bool((d <= bf16_ulp(torch.maximum(x1.double().abs(), x2.double().abs()))).all()), float(d.max())
    # and against float64: C = R + a @ W^T, xn = the RMSNorm of that C
    ref = res.double() + a.double() @ w.double().t()
    assert_within(c1, ref, C_DOT * K * U * (a.double().abs() @ w.double().abs().t()) + U * ref.abs() + 2 * U * res.double().abs(),
                   "C")
    xr = _rms64(c1, gamma, eps)
    assert_within(x1, xr, bf16_ulp(torch.maximum(xr.abs(), x1.double().abs())), "xn")

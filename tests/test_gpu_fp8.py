"""`-m gpu`: the opt-in FP8 weight mode of the LLM decoder (include/icl_hip.h icl_pack_fp8_weights / icl_gemm_fp8w).

The mode is defined as "the bf16 model with every decoder GEMM weight replaced by its FP8 rounding W' = q * 2^e_n", so every check
here is exact: the packer's bytes against torch's own e4m3fn rounding, the fp8-weight decode kernel against the bf16 tile-6 kernel
on the decode-packed copy of W' (bit-identical), and a model in fp8 mode against a bf16-mode model given the same W'."""
import json
import os

import pytest
import torch

from decoder_support import same_generation, stream_prompts
from fp8_ref import ref_pack, ref_q
from fp64_bounds import C_DOT, U, _dot, assert_within, bf16_ulp
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _weights(N, K, seed, scale=0.02):
    g = torch.Generator(device=DEV).manual_seed(seed)
    # rows of very different magnitudes: every row gets its own exponent
    rows = torch.exp2(torch.randint(-12, 4, (N, 1), device=DEV, generator=g).float())
    return (torch.randn(N, K, device=DEV, generator=g) * scale * rows).to(torch.bfloat16)


# Llama-2-7B and Qwen2-7B decoder shapes (qkv with the 64 LoRA-augmentation columns of k_aug)
SHAPES = {
    "llama7b": dict(qkv=(3 * 4096, 4096 + 64), o=(4096, 4096), gu=(2 * 11008, 4096), down=(4096, 11008)),
    "qwen2_7b": dict(qkv=(3 * 3584, 3584 + 64), o=(3584, 3584), gu=(2 * 18944, 3584), down=(3584, 18944)),
}


@pytest.mark.parametrize("model", sorted(SHAPES))
@pytest.mark.parametrize("which", ["qkv", "o", "gu", "down"])
def test_packer_matches_torch_reference(B, model, which):
    N, K = SHAPES[model][which]
    w = _weights(N, K, seed=sorted(SHAPES).index(model) * 4 + ["qkv", "o", "gu", "down"].index(which))
    src = w.clone()
    q, s, wd = B.pack_fp8_weights(w)
    rq, rs, rwd = ref_q(w)
    assert torch.equal(s, rs)
    assert torch.equal(q, ref_pack(rq))
    assert torch.equal(wd.view(torch.int16), rwd.view(torch.int16))
    assert torch.equal(w.view(torch.int16), src.view(torch.int16))     # the source is left alone (out-of-place form)


def test_packer_ragged_zero_row_tiny_row_and_in_place(B):
    N, K = 1000, 576
    w = _weights(N, K, seed=5)
    w[7] = 0
    w[8] = 1e-30
    w[9, ::3] = -1e-30
    w[10, 5] = 448.0                       # exactly the top of the e4m3 range: e = 0
    w[11, 5] = 452.0                       # just above (bf16 has no 449): e = 1
    q, s, wd = B.pack_fp8_weights(w)
    rq, rs, rwd = ref_q(w)
    assert float(s[7]) == 1.0 and float(s[10]) == 1.0 and float(s[11]) == 2.0
    assert torch.equal(s, rs) and torch.equal(q, ref_pack(rq))      # ref_pack zero-fills the padding rows of the last block
    assert torch.equal(wd.view(torch.int16), rwd.view(torch.int16))
    # W' as q.float() * 2^e, exactly
    assert torch.equal(wd.float(), (rq.view(torch.float8_e4m3fn).float() * rs[:, None]).to(torch.bfloat16).float())
    # in place: W' overwrites the source, same bytes
    w2 = w.clone()
    q2, s2, out = B.pack_fp8_weights(w2, out=w2)
    assert out.data_ptr() == w2.data_ptr() and torch.equal(q2, q) and torch.equal(s2, s)
    assert torch.equal(w2.view(torch.int16), rwd.view(torch.int16))
    # re-quantizing W' gives W' again
    _, _, wdd = B.pack_fp8_weights(wd)
    assert torch.equal(wdd.view(torch.int16), wd.view(torch.int16))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_packer_rejects_non_finite(B, bad):
    w = _weights(64, 128, seed=1)
    w[33, 77] = bad
    with pytest.raises(B.IclError, match="non-finite"):
        B.pack_fp8_weights(w)


def test_every_finite_e4m3_code_reads_back_exactly(B):
    """All 254 finite e4m3fn codes (subnormals, both zeros and both signs included), at scale 1 and at scale 2^-20, through the
    packer and the fp8-weight kernel against one-hot activations: the kernel's output is W' itself."""
    codes = torch.tensor([c for c in range(256) if c not in (0x7F, 0xFF)], dtype=torch.uint8)
    vals = codes.view(torch.float8_e4m3fn).float()
    assert vals.numel() == 254 and torch.isfinite(vals).all()
    K = 64
    w = torch.zeros(2 * 256, K)
    for blk, e in enumerate((0, -20)):
        rows = slice(blk * 256, blk * 256 + 254)
        w[rows, 0] = 448.0 * 2.0 ** e          # pins the row scale to 2^e
        w[rows, 1] = vals * 2.0 ** e
    w = w.to(torch.bfloat16).to(DEV)
    q, s, wd = B.pack_fp8_weights(w)
    assert torch.equal(wd.float(), w.float())                       # every value is already its own FP8 rounding
    rq = ref_q(w)[0]
    assert torch.equal(rq[:254, 1].cpu(), codes) and torch.equal(q, ref_pack(rq))
    a = torch.zeros(2, K, dtype=torch.bfloat16, device=DEV)
    a[0, 0] = 1
    a[1, 1] = 1
    out = torch.empty(2, w.shape[0], dtype=torch.float32, device=DEV)
    B.gemm(a, q, out, w_scale=s, N=w.shape[0], K=K)
    assert torch.equal(out, w.float().t()[:2])


# ---- the fp8-weight kernel against tile 6 on the decode-packed W' ------------------------------------------------------
_CACHE = {}


def _packed(B, model, which):
    key = (model, which)
    if key not in _CACHE:
        N, K = SHAPES[model][which]
        w = _weights(N, K, seed=len(_CACHE) + 11)
        q, s, wd = B.pack_fp8_weights(w)
        del w
        _CACHE.clear()                     # one matrix resident at a time
        _CACHE[key] = (q, s, wd, B.pack_decode_weights(wd))
    return _CACHE[key]


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30))


CASES = [(model, epi) for model in sorted(SHAPES) for epi in ("none", "bias", "swiglu", "residual", "rmsnorm")]


@pytest.mark.parametrize("model,epi", CASES)
def test_fp8w_kernel_is_bit_identical_to_tile6_on_w_prime(B, model, epi):
    which = {"none": "qkv", "bias": "qkv", "swiglu": "gu", "residual": "down", "rmsnorm": "o"}[epi]
    q, s, wd, dp = _packed(B, model, which)
    N, K = SHAPES[model][which]
    g = torch.Generator(device=DEV).manual_seed(N + K)
    for M in (1, 2, 5, 8, 24, 64):
        a = (torch.randn(M, K, device=DEV, generator=g)).to(torch.bfloat16)
        if epi == "none":
            o8, o6 = (torch.empty(M, N, dtype=torch.bfloat16, device=DEV) for _ in range(2))
            B.gemm(a, q, o8, w_scale=s, N=N, K=K)
            B.gemm(a, dp, o6, tile=6, N=N, K=K)
            ref, tol = a.float() @ wd.float().t(), 4e-3
        elif epi == "bias":
            bias = torch.randn(N, device=DEV, generator=g)
            o8, o6 = (torch.empty(M, N, dtype=torch.bfloat16, device=DEV) for _ in range(2))
            B.gemm(a, q, o8, bias=bias, w_scale=s, N=N, K=K)
            B.gemm(a, dp, o6, bias=bias, tile=6, N=N, K=K)
            ref, tol = a.float() @ wd.float().t() + bias, 4e-3
        elif epi == "swiglu":
            o8, o6 = (torch.empty(M, N // 2, dtype=torch.bfloat16, device=DEV) for _ in range(2))
            B.gemm(a, q, o8, swiglu=True, w_scale=s, N=N, K=K)
            B.gemm(a, dp, o6, swiglu=True, tile=6, N=N, K=K)
            y = (a.float() @ wd.float().t()).view(M, N // 32, 2, 16)
            ref, tol = (torch.nn.functional.silu(y[:, :, 0]) * y[:, :, 1]).reshape(M, N // 2), 4e-3
        elif epi == "residual":
            r = torch.randn(M, N, device=DEV, generator=g)
            o8, o6 = (torch.empty(M, N, dtype=torch.float32, device=DEV) for _ in range(2))
            B.gemm(a, q, o8, residual=r, w_scale=s, N=N, K=K)
            B.gemm(a, dp, o6, residual=r, tile=6, N=N, K=K)
            ref, tol = a.float() @ wd.float().t() + r, 1e-3
        else:   # the gemm_rmsnorm pairing: h = R + a W'^T (f32) and xn = bf16(rmsnorm(h) * gamma)
            r = torch.randn(M, N, device=DEV, generator=g)
            gamma = 1 + 0.1 * torch.randn(N, device=DEV, generator=g)
            o8, o6 = (torch.empty(M, N, dtype=torch.float32, device=DEV) for _ in range(2))
            x8, x6 = (torch.empty(M, N, dtype=torch.bfloat16, device=DEV) for _ in range(2))
            B.gemm_rmsnorm(a, q, o8, gamma, 1e-5, x8, residual=r, w_scale=s, N=N, K=K)
            B.gemm_rmsnorm(a, dp, o6, gamma, 1e-5, x6, residual=r, tile=6, N=N, K=K)
            assert torch.equal(x8.view(torch.int16), x6.view(torch.int16)), (model, M)
            ref, tol = a.float() @ wd.float().t() + r, 1e-3
            hn = ref * torch.rsqrt(ref.pow(2).mean(1, keepdim=True) + 1e-5) * gamma
            assert _rel(x8, hn) < 4e-3
        bits = torch.int16 if o8.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(o8.view(bits), o6.view(bits)), (model, epi, M)
        err = _rel(o8, ref)
        assert err < tol, (model, epi, M, err)


@pytest.mark.parametrize("K", [64, 192, 576])
def test_fp8w_tile6_tile4_bit_identical_on_small_shapes(B, K):
    """The three weight forms of the skinny kernel (fp8 decode-packed, tile 6 on the decode-packed W', tile 4 on row-major W') at
    the sizes where their K walks differ most: K = 64 / 192 / 576 gives waves an empty k-step range, a single half-pair, and ranges
    that start or end inside a k-pair; N = 40 / 264 / 96 leaves the last n-tile ragged or absent; M covers 1, 2 and 4 row blocks.
    Outputs start as NaN, and the fp8 form is held to the per-element fp64 bound of test_gpu_decode_plan.py, so the three cannot agree
    on a wrong answer."""
    g = torch.Generator(device=DEV).manual_seed(77 + K)
    for epi, Ns in (("plain", (16, 40, 264)), ("bias_res", (16, 40, 264)), ("swiglu", (32, 96))):
        for N in Ns:
            q, s, wd = B.pack_fp8_weights(_weights(N, K, seed=N + K))
            dp = B.pack_decode_weights(wd)
            w64 = wd.double()
            w64a = w64.abs()
            for M in (1, 17, 33, 64):
                what = (K, epi, N, M)
                a = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
                if epi == "plain":
                    kw, odt, nout = {}, torch.bfloat16, N
                    ref, mag = _dot(a, w64, w64a)
                    bound = C_DOT * K * U * mag + U * ref.abs()
                elif epi == "bias_res":
                    bias = torch.randn(N, device=DEV, generator=g)
                    r = torch.randn(M, N, device=DEV, generator=g)
                    kw, odt, nout = dict(bias=bias, residual=r), torch.float32, N
                    ref, mag = _dot(a, w64, w64a)
                    ref = ref + bias.double() + r.double()
                    bound = C_DOT * K * U * mag + U * ref.abs() + 2 * U * (bias.double().abs() + r.double().abs())
                else:
                    kw, odt, nout = dict(swiglu=True), torch.bfloat16, N // 2
                    gv, uv = (w64.view(N // 32, 2, 16, K)[:, i].reshape(nout, K) for i in range(2))
                    gate, gmag = _dot(a, gv, gv.abs())
                    up, umag = _dot(a, uv, uv.abs())
                    sg = gate * torch.sigmoid(gate)
                    ref = sg * up
                    eg = C_DOT * K * U * gmag + U * gate.abs()
                    eu = C_DOT * K * U * umag + U * up.abs()
                    bound = 1.1 * eg * (up.abs() + eu) + sg.abs() * eu + U * (16 + 4 * gate.abs()) * ref.abs()
                o8, o6, o4 = (torch.full((M, nout), float("nan"), dtype=odt, device=DEV) for _ in range(3))
                B.gemm(a, q, o8, w_scale=s, N=N, K=K, **kw)
                B.gemm(a, dp, o6, tile=6, N=N, K=K, **kw)
                B.gemm(a, wd, o4, tile=4, N=N, K=K, **kw)
                if odt == torch.bfloat16:
                    bound = bound + bf16_ulp(torch.maximum(ref.abs(), o8.double().abs()))
                assert_within(o8, ref, bound, f"fp8w {what}")
                bits = torch.int16 if odt == torch.bfloat16 else torch.int32
                assert torch.equal(o8.view(bits), o6.view(bits)), ("fp8w != tile 6", what)
                assert torch.equal(o4.view(bits), o6.view(bits)), ("tile 4 != tile 6", what)


def test_fp8w_kernel_argument_checks(B):
    q, s, wd, dp = _packed(B, "llama7b", "o")
    a = torch.zeros(65, 4096, dtype=torch.bfloat16, device=DEV)
    out = torch.empty(65, 4096, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(B.IclError, match="M <= 64"):
        B.gemm(a, q, out, w_scale=s, N=4096, K=4096)


# ---- model level: fp8 mode == the bf16 model on W' ------------------------------------------------------------------------
def _pair(kind):
    """(runtime in fp8 mode, runtime in bf16 mode holding the fp8 runtime's W' matrices)."""
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import QwenAudioCfg, SalmonnCfg
    if kind == "salmonn":
        from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime as R
        cfg = SalmonnCfg.tiny(use_beats=True, lora=True)
        sd = synth.salmonn_state(cfg, seed=0, jitter=True)
        lm = cfg.llama
    else:
        from icl_speech_text_llm_amd.runtime.qwen import QwenAudioRuntime as R
        cfg = QwenAudioCfg.tiny(lora=True)
        sd = synth.qwen_audio_state(cfg, seed=0)
        lm = cfg.llm
    r8 = R(cfg, dict(sd), device=DEV, llm_weight_dtype="fp8")
    rb = R(cfg, dict(sd), device=DEV)
    for L8, Lb in zip(r8.llama.w.layers, rb.llama.w.layers):
        assert L8.decode_packed is None and L8.fp8 is not None           # no bf16 decode copy is made at load in fp8 mode
        for (q, s), name in zip(L8.fp8, ("wqkv", "wo", "wgu", "wdown")):
            rq, rs, rwd = ref_q(getattr(Lb, name))
            assert torch.equal(getattr(L8, name).view(torch.int16), rwd.view(torch.int16)), name
            assert torch.equal(s, rs) and torch.equal(q, ref_pack(rq)), name
            setattr(Lb, name, getattr(L8, name).clone())
        Lb.decode_packed = None
    rb.llama.ensure_decode_packed()
    return r8, rb, lm


@pytest.fixture(scope="module", params=["salmonn", "qwen2"])
def pair(request):
    return _pair(request.param)


@pytest.mark.parametrize("lens", [[37], [33, 90, 61, 12, 5, 70, 44, 21], [9 + 7 * i for i in range(16)]])
def test_model_greedy_matches_bf16_on_w_prime(pair, lens):
    r8, rb, lm = pair
    prompts = stream_prompts(lm.vocab, lens, seed=len(lens))
    kw = dict(max_new_tokens=8, suppress_eos=True, want_first_logits=True)
    same_generation(r8.generate(prompts, None, **kw), rb.generate(prompts, None, **kw))


def test_model_sampled_and_beam_match_bf16_on_w_prime(pair):
    r8, rb, lm = pair
    prompts = stream_prompts(lm.vocab, [40, 23], seed=3)
    outs = []
    for rt in (r8, rb):
        gen = torch.Generator(device=DEV).manual_seed(1234)
        outs.append(rt.generate(prompts, None, max_new_tokens=8, do_sample=True, temperature=0.8, top_p=0.9, top_k=50,
                                generator=gen, want_first_logits=True, suppress_eos=True))
    same_generation(*outs)
    beams = [rt.generate(prompts[:1], None, max_new_tokens=6, suppress_eos=True, num_beams=4, want_first_logits=True) for rt in (r8, rb)]
    same_generation(*beams)


def test_model_forward_logits_match_bf16_on_w_prime(pair):
    r8, rb, lm = pair
    prompts = stream_prompts(lm.vocab, [37, 150, 64], seed=9)
    l8, n8 = r8.forward_logits(prompts, None)
    l8 = l8.clone()
    lb, nb = rb.forward_logits(prompts, None)
    assert n8 == nb and torch.equal(l8, lb)


def test_fp8_decode_differs_from_bf16_only_by_the_weight_rounding(pair):
    """Sanity in the other direction: fp8 mode is NOT the bf16 model (the weights really were rounded), and its first-step logits
    stay within a few percent of the unrounded model's."""
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import QwenAudioCfg, SalmonnCfg
    r8, rb, lm = pair
    if hasattr(r8, "tower"):
        from icl_speech_text_llm_amd.runtime.qwen import QwenAudioRuntime as R
        cfg = QwenAudioCfg.tiny(lora=True)
        orig = R(cfg, synth.qwen_audio_state(cfg, seed=0), device=DEV)
    else:
        from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime as R
        cfg = SalmonnCfg.tiny(use_beats=True, lora=True)
        orig = R(cfg, synth.salmonn_state(cfg, seed=0, jitter=True), device=DEV)
    prompts = stream_prompts(lm.vocab, [50], seed=4)
    a = r8.generate(prompts, None, max_new_tokens=1, suppress_eos=True, want_first_logits=True).first_logits
    b = orig.generate(prompts, None, max_new_tokens=1, suppress_eos=True, want_first_logits=True).first_logits
    err = _rel(a, b)
    print(f"fp8 mode vs bf16 weights: first-step logits rel-L2 {err:.2e}")
    assert 0 < err < 0.1


# ---- plugin / CLI ---------------------------------------------------------------------------------------------------------
def _w_prime_state_dict(model):
    """The fp8 runtime's W' matrices under the checkpoint's own key names (q/k/v and LoRA B split back out of wqkv, gate/up
    de-interleaved), i.e. a checkpoint that makes a bf16-mode model compute on W'."""
    rt = model.runtime
    c, w = model.cfg.llama, rt.llama.w
    h, I, r = c.hidden, c.ffn, c.lora_rank
    sd = {}
    for i, L in enumerate(w.layers):
        p = f"llama_model.model.layers.{i}."
        for j, n in enumerate(("q_proj", "k_proj", "v_proj")):
            sd[p + f"self_attn.{n}.weight"] = L.wqkv[j * h:(j + 1) * h, :h].cpu()
        for ti, tgt in enumerate(c.lora_targets):
            j = ("q_proj", "k_proj", "v_proj").index(tgt)
            sd[p + f"self_attn.{tgt}.lora_B.weight"] = L.wqkv[j * h:(j + 1) * h, h + ti * r:h + (ti + 1) * r].cpu()
        gu = L.wgu.view(I // 16, 2, 16, h)
        sd[p + "mlp.gate_proj.weight"] = gu[:, 0].reshape(I, h).cpu()
        sd[p + "mlp.up_proj.weight"] = gu[:, 1].reshape(I, h).cpu()
        sd[p + "self_attn.o_proj.weight"] = L.wo.cpu()
        sd[p + "mlp.down_proj.weight"] = L.wdown.cpu()
    return sd


def test_plugin_fp8_mode_and_reload_requantizes():
    from icl_speech_text_llm_amd.config.inference_config import get_inference_config
    from icl_speech_text_llm_amd.models.model_factory import ModelFactory
    args = dict(get_inference_config("salmonn")["model_args"], arch="tiny")
    m = ModelFactory.create_model("salmonn", device=DEV, low_resource=True, llm_weight_dtype="fp8", **args)
    assert m.runtime.llama.weight_dtype == "fp8"
    # a later weight load re-quantizes: perturb every decoder weight, load, and the new W' is the rounding of the NEW weights
    sd = {k: v for k, v in m.salmonn.state_dict().items() if k.startswith("llama_model.model.layers.")}
    g = torch.Generator().manual_seed(0)
    new = {k: (v.float() * (1 + 0.5 * torch.rand(v.shape, generator=g))).to(torch.bfloat16) for k, v in sd.items()
           if k.endswith("proj.weight")}
    m.load_state_dict(new, strict=False)
    L = m.runtime.llama.w.layers[0]
    assert torch.equal(L.wo.view(torch.int16), ref_q(new["llama_model.model.layers.0.self_attn.o_proj.weight"].to(DEV))[2].view(torch.int16))
    wsd = _w_prime_state_dict(m)
    assert torch.equal(wsd["llama_model.model.layers.0.mlp.up_proj.weight"].view(torch.int16),
                       ref_q(new["llama_model.model.layers.0.mlp.up_proj.weight"].to(DEV))[2].cpu().view(torch.int16))


def test_cli_fp8_writes_the_same_files_as_bf16_on_w_prime(tmp_path):
    from icl_speech_text_llm_amd.config.inference_config import get_inference_config
    from icl_speech_text_llm_amd.inference.inference import main
    from icl_speech_text_llm_amd.models.model_factory import ModelFactory
    args = dict(get_inference_config("salmonn")["model_args"], arch="tiny")
    m = ModelFactory.create_model("salmonn", device=DEV, low_resource=True, llm_weight_dtype="fp8", **args)
    ckpt = tmp_path / "w_prime.pt"
    torch.save({"model": _w_prime_state_dict(m)}, ckpt)
    del m
    common = ["--run_name", "t", "--dataset_type", "voxceleb-hvb", "--arch", "tiny", "--synthetic_items", "3", "--batch_size", "1",
              "--num_workers", "0", "--device", "cuda"]
    outs = {}
    for tag, extra in (("fp8", ["--peft_model_path", "", "--llm_weights", "fp8"]),
                       ("bf16", ["--peft_model_path", str(ckpt), "--llm_weights", "bf16"])):
        out = tmp_path / tag
        assert main(common + extra + ["--results_dir", str(out)]) == 0
        files = sorted(os.listdir(out))
        outs[tag] = {f: json.load(open(out / f)) for f in files if f.endswith(("_results.json", "_metrics.json"))}
        assert len(outs[tag]) == 2
    res = [v for k, v in outs["fp8"].items() if k.endswith("_results.json")][0]
    assert len(res) == 6
    assert outs["fp8"] == outs["bf16"]

"""Every stage of the LLM decoder chain on the kernels, per element against float64 (`-m gpu`; all input goes through
runtime/binding.py).  tests/decoder_stage_check.py records what each launch of LlamaHIP.embed / prefill / _last_layer_rows /
decode_step / logits wrote — a before and an after copy of the whole storage behind every written argument — and judges it
against the float64 specification of that stage (oracle/decoder_stages.py: the model definition applied to the state dict and to
the logical contents of the previous stage's ACTUAL output) with the bound that kernel family already has: errors do not
accumulate over the chain, so no tolerance is introduced here.  What a launch must not write (the LoRA columns and the zero tail
of the input buffer, the k / v columns of the QKV buffer under a cache-appending epilogue, every other row of every cache plane
in every layer) must keep its bits; caches and never-zeroed workspace buffers start as NaN.  The three fused launch kinds are
judged through a replay of their two-launch form plus bit equality.  The reference never sees a launch's strides, offsets,
``pos`` / ``sid`` / ``lens`` or the cache's geometry: the host code that places the operands is under test together with the
kernels.  tests/test_decoder_stages.py runs the same check without a GPU on an emulation of the wrappers and shows that twenty
planted host-side mistakes are rejected at the stage they are planted in.

Cases (state dicts: synth.llama_state(..., jitter=True); prompts: decoder_support.row_prompts; every model has 2 layers):
  tiny families  (a) SalmonnCfg.tiny().llama, (b) QwenAudioCfg.tiny().llm (QKV bias, LoRA on q / k), (c) 4 heads of 64 (no RoPE
                 epilogue, no trimmed layer), (d) grouped-query (a), (e) QK-norm multi-head and grouped, (f) (a) without LoRA.
                 Prefill over the ragged lengths 1, 5, 64, 65, 200 with a cache and last rows only (trimmed on a, b, f), untrimmed,
                 full height, without a cache, an FP8 cache (a, c), two chunks through cache.rows(); three consecutive decode steps
                 (one row crosses 63 -> 64 -> 65, one ends at max_len - 1) at 65, 9, 1 rows — on (a) also 64 and 8, FP8 weights,
                 an FP8 KV cache, both, and each of the three decode switches off.  One runtime and workspace per family, largest
                 batch first.
  fused epilogue hidden 1024 (8 heads of 128), 3079 packed rows of prompts up to 400 positions: the QKV GEMM on the 256 tile with
                 the RoPE epilogue into a bf16 cache, with an FP8 cache, without a cache, and last rows only.
  plan width     the Llama-2-7B shape, 2 layers, max_len 16, one decode step: 8 rows with FP8 weights (icl_gemm_fp8w), 129 and
                 256 rows (every site split-K on the 256 tile), 257 rows (the 64x64 tile, split-K o / down).

Worst err / bound per stage kind measured on MI355X: DESIGN.md."""
import dataclasses

import pytest
import torch

import decoder_stage_check as sc
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)
from oracle import decoder_stages as ds

pytestmark = pytest.mark.gpu

_ENV = {}


def _make(cfg, prefix, key, weight_dtype="bf16", dtype=torch.float32, **switches):
    from icl_speech_text_llm_amd.runtime import engines as E, packing as P, synth
    if key not in _ENV:
        sd = synth.llama_state(cfg, synth._Gen(0, DEV, dtype, jitter=True), prefix=prefix)
        rt = E.LlamaHIP(P.pack_llama(dict(sd), cfg, DEV, prefix=prefix), DEV, weight_dtype=weight_dtype)
        for k, v in switches.items():
            setattr(rt, k, v)
        ds.check_packed_llama(sd, rt, prefix)
        walk_sd = ds.w_prime_state(sd, cfg, prefix) if weight_dtype == "fp8" else sd
        _ENV[key] = (cfg, prefix, sd, walk_sd, rt, E.Workspace(DEV))
    return _ENV[key]


def _env(name, weight_dtype="bf16", **switches):
    cfg, prefix = sc.family_cfg(name)
    return _make(cfg, prefix, (name, weight_dtype, tuple(sorted(switches.items()))), weight_dtype, **switches)


def _decode(env, Bn, tag, **kw):
    cfg, prefix, sd, walk_sd, rt, ws = env
    worst, counts = sc.run_decode(rt, ws, sd, prefix, Bn, sd_walk=walk_sd, **kw)
    sc.report(f"{tag} decode {Bn}", worst)
    assert max(worst.values()) <= 1.0
    return counts


def _prefill(env, tag, lens=None, **kw):
    cfg, prefix, sd, walk_sd, rt, ws = env
    worst, count, form, _ = sc.run_prefill(rt, ws, walk_sd, prefix, lens or sc.PREFILL_LENS, **kw)
    sc.report(f"{tag} prefill", worst)
    assert max(worst.values()) <= 1.0
    return count, form


def decode_launches(cfg, Bn, fuse_rope=True, fuse_norms=True):
    """Launches of one decode step of a 2-layer decoder: the embedding, per layer [input norm] [LoRA down] QKV, one or two
    launches of RoPE + attention, o (+ norm), gate/up, down (+ norm), then [final norm] LM head."""
    two = not (fuse_rope and Bn > 8 and not cfg.qk_norm and cfg.group == 1)
    per = 1 + (1 if cfg.lora_rank else 0) + 1 + (2 if two else 1) + (3 if fuse_norms else 4)
    return 1 + 2 * per - (1 if fuse_norms else 0) + (1 if fuse_norms else 2)


def _full(cfg):
    """embed, two layers of norm [LoRA down] QKV RoPE attention o norm gate/up down, final norm + LM head."""
    return 1 + 2 * (8 + (1 if cfg.lora_rank else 0)) + 2


FAMILIES = ("a", "b", "c", "d", "e", "e_gqa", "f")
TRIMS = ("a", "b", "f")                       # head_dim 128, multi-head, no q / k norm: the trimmed last layer
DECODES = [(f, Bn) for f in FAMILIES for Bn in ((65, 64, 9, 8, 1) if f == "a" else (65, 9, 1))]
PREFILLS = [(f, form) for f in FAMILIES for form in ("last_rows", "untrimmed", "full_height", "no_cache", "fp8_cache", "two_chunks")
            if form != "fp8_cache" or f in ("a", "c")]


@pytest.mark.parametrize("name,Bn", DECODES)
def test_tiny_decode(B, name, Bn):
    env = _env(name)
    assert _decode(env, Bn, name) == [decode_launches(env[0], Bn)] * 3


@pytest.mark.parametrize("name,form", PREFILLS)
def test_tiny_prefill(B, name, form):
    env = _env(name)
    cfg, rt = env[0], env[4]
    full, trims = _full(cfg), name in TRIMS
    if form == "last_rows":
        count, f = _prefill(env, name + " last rows", kv="bf16", last_rows_only=True, speech_rows=10 if name == "a" else 0)
        assert f["trim"] == trims and not f["epilogue"] and count == (full + 2 if trims else full + 1)
    elif form == "untrimmed":
        rt.prefill_last_rows = False
        try:
            count, f = _prefill(env, name + " untrimmed", kv="bf16", last_rows_only=True)
        finally:
            del rt.prefill_last_rows
        assert not f["trim"] and count == full + 1
    elif form == "full_height":
        assert _prefill(env, name + " full height", kv="bf16")[0] == full
    elif form == "no_cache":
        assert _prefill(env, name + " no cache")[0] == full
    elif form == "fp8_cache":
        assert _prefill(env, name + " fp8 cache", kv="fp8")[0] == full + 2            # + one kv_append_fp8 per layer
    else:
        count, f = _prefill(env, name + " two chunks", kv="bf16", chunk=2)
        assert count == 2 * (full - 3 + (2 if trims else 1))                          # no embed, no logits inside the chunks


@pytest.mark.parametrize("Bn", (65, 64, 9, 8, 1))
@pytest.mark.parametrize("weights,kv", [("fp8", "bf16"), ("bf16", "fp8"), ("fp8", "fp8")])
def test_a_fp8_modes(B, weights, kv, Bn):
    """FP8 weights (the walk reads W', which check_packed_llama has shown to be the FP8 rounding of W), an FP8 KV cache in the
    workspace that has held the bf16 one, and both."""
    env = _env("a", weights)
    rt = env[4]
    if kv == "fp8" and Bn == 65:
        _decode(env, 9, f"a w={weights} kv=bf16 first")
    if weights == "fp8":
        assert all((p.tile == "fp8w") == (Bn <= 8) for n, p in rt.decode_plan(Bn).sites.items() if n != "lm_head")
    assert _decode(env, Bn, f"a w={weights} kv={kv}", kv=kv) == [decode_launches(env[0], Bn)] * 3


@pytest.mark.parametrize("Bn", (65, 64, 9, 8, 1))
@pytest.mark.parametrize("switch", ["fuse_decode_rope", "fuse_decode_norms", "decode_packed_weights"])
def test_a_switches(B, switch, Bn):
    env = _env("a", **{switch: False})
    want = decode_launches(env[0], Bn, fuse_rope=switch != "fuse_decode_rope", fuse_norms=switch != "fuse_decode_norms")
    assert _decode(env, Bn, f"a {switch}=False") == [want] * 3


# ---- the QKV GEMM on the 256 tile with the RoPE epilogue -----------------------------------------------------------------------
EPILOGUE_LENS = [400, 399, 385, 384, 383, 321, 257, 400, 150]        # 3079 packed rows: the smallest filled grid is 3073


def _epilogue_env():
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    cfg = dataclasses.replace(SalmonnCfg.tiny().llama, hidden=1024, n_heads=8, ffn=2048)
    return _make(cfg, "llama_model.", "epilogue")


@pytest.mark.parametrize("form", ["in_cache", "fp8_cache", "no_cache", "last_rows"])
def test_fused_epilogue_prefill(B, form):
    env = _epilogue_env()
    cfg, rt = env[0], env[4]
    M = sum(EPILOGUE_LENS)
    assert B.rope_fusable(M, cfg.n_heads, cfg.head_dim, rt.w.k_aug) and not B.rope_fusable(M - 7, cfg.n_heads, cfg.head_dim, rt.w.k_aug)
    full = 1 + 2 * 8 + 2                        # embed, two layers of norm LoRA QKV+RoPE attention o norm gate/up down, logits
    kw = dict(in_cache=dict(kv="bf16"), fp8_cache=dict(kv="fp8"), no_cache=dict(), last_rows=dict(kv="bf16", last_rows_only=True))[form]
    count, f = _prefill(env, "epilogue " + form, lens=EPILOGUE_LENS, want_logits=form == "last_rows", **kw)
    assert f["epilogue"] and f["trim"] == (form == "last_rows")
    assert count == {"in_cache": full - 2, "fp8_cache": full - 2 + 2, "no_cache": full - 2, "last_rows": full + 3}[form]


# ---- the decode plan at full width: split-K at every site, the 256 tile above 128 rows, the fp8-weight kernel at 8 rows ------------
def _wide_env(weight_dtype):
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    cfg = dataclasses.replace(SalmonnCfg.llama2_7b().llama, n_layers=2)
    if ("wide", weight_dtype) not in _ENV:      # one full-width runtime at a time
        for k in [k for k in _ENV if k[0] == "wide"]:
            del _ENV[k]
        torch.cuda.empty_cache()
    return _make(cfg, "llama_model.", ("wide", weight_dtype), weight_dtype, dtype=torch.bfloat16)


@pytest.mark.parametrize("Bn,weights", [(257, "bf16"), (256, "bf16"), (129, "bf16"), (8, "fp8")])
def test_plan_width_decode_step(B, Bn, weights):
    env = _wide_env(weights)
    cfg, rt = env[0], env[4]
    sites = {n: p for n, p in rt.decode_plan(Bn).sites.items() if n != "lm_head"}
    if Bn == 8:
        assert all(p.tile == "fp8w" and p.weight == "fp8" for p in sites.values())
    elif Bn <= 256:
        assert all(p.tile == 3 and p.split_k > 1 for p in sites.values()) and rt.decode_plan(Bn).workspace > 0
    else:
        assert all(p.tile == 2 for p in sites.values()) and sites["o"].split_k > 1 and sites["down"].split_k > 1
    plens = [(3, 1, 5, 2, 4)[b % 5] for b in range(Bn - 1)] + [15]
    counts = _decode(env, Bn, f"7B-shape w={weights}", steps=1, prompt_lens=plens, max_len=16)
    assert counts == [decode_launches(cfg, Bn)]

"""CPU: QK-norm decoders (Qwen3) — the per-head q / k RMSNorm between the projection and RoPE.

  * QKNormOracle (tests/qknorm_ref.py) is pinned to transformers' Qwen3ForCausalLM by tests/golden/qwen3_tiny.npz
    (tests/golden/make_qwen3_golden.py) at the bounds of test_llama_forward_loss_and_generate_match_hf, and the plain LlamaOracle
    on the same weights misses by more than 100x that bound: the fixture can tell.
  * The norm bound of qknorm_ref_bound: an f32 emulation of icl_qknorm_rope_kv_bf16 in the kernel's order passes the two-stage
    check of test_gpu_qknorm.py on that test's inputs, and each one-mistake variant fails it.
  * Configuration, packing, synthetic weights, the stray-key and FP8-KV refusals, the plugin's state_dict round trip, the symbol."""
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import qknorm_ref as qr

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOGIT_TOL, LOSS_TOL = 2e-4, 1e-4            # test_llama_forward_loss_and_generate_match_hf


# ---- the HF pin -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qwen3():
    a = np.load(os.path.join(G, "qwen3_tiny.npz"))
    sd = {k[2:]: torch.from_numpy(a[k].view(np.int16)).view(torch.bfloat16).float() for k in a.files if k.startswith("w:")}
    return a, sd


def test_golden_file_is_small_and_has_nontrivial_gains(qwen3):
    a, sd = qwen3
    assert os.path.getsize(os.path.join(G, "qwen3_tiny.npz")) < 1 << 20
    for i in range(2):
        gq, gk = (sd[f"model.layers.{i}.self_attn.{n}_norm.weight"] for n in "qk")
        assert gq.shape == gk.shape == (128,) and float((gq - 1).abs().max()) > 0.3 and float((gq - gk).abs().max()) > 0.3
    assert sd["model.layers.0.self_attn.q_proj.weight"].shape == (256, 256)
    assert sd["model.layers.0.self_attn.k_proj.weight"].shape == (128, 256)


def test_qknorm_oracle_matches_qwen3_for_causal_lm(qwen3):
    a, sd = qwen3
    llm = qr.QKNormOracle(sd, n_heads=2, rms_eps=1e-6, n_kv_heads=1)
    emb, labels = torch.from_numpy(a["emb"]), torch.from_numpy(a["labels"])
    logits, loss = llm.forward(emb, labels)
    err = float(np.abs(logits.numpy() - a["logits"]).max())
    print(f"QKNormOracle vs Qwen3ForCausalLM: logits max abs {err:.2e} at max |logit| {float(np.abs(a['logits']).max()):.2f}, "
          f"loss {abs(float(loss) - float(a['loss'])):.2e}")
    assert err < LOGIT_TOL
    assert abs(float(loss) - float(a["loss"])) < LOSS_TOL
    assert llm.generate_greedy(emb, a["gen"].shape[1], eos_id=-1, pad_id=47).tolist() == a["gen"].tolist()


def test_plain_oracle_misses_the_qwen3_golden(qwen3):
    from oracle import models as om
    a, sd = qwen3
    logits, _ = om.LlamaOracle(sd, n_heads=2, rms_eps=1e-6, n_kv_heads=1).forward(torch.from_numpy(a["emb"]))
    err = float(np.abs(logits.numpy() - a["logits"]).max())
    print(f"LlamaOracle without the q / k norm vs Qwen3ForCausalLM: logits max abs {err:.2e}")
    assert err > 100 * LOGIT_TOL


# ---- the norm bound: the kernel's order passes, one mistake fails ------------------------------------------------------------------
SHAPES = [(5, 4, 1, 128), (2, 32, 8, 128), (5, 16, 16, 64), (1, 32, 1, 64)]      # (M, H, Hkv, D), from test_gpu_qknorm.py
MAX_LEN = 16
MUTANTS = ["no_eps", "mean_2d", "mean_half", "k_with_q_gamma", "gamma_by_chunk", "norm_after_rope", "no_bf16_round", "v_normed"]


def positions(M):
    """The positions of stage 2 of test_gpu_qknorm.py: in range, not monotonic, never 0."""
    return torch.tensor([1 + (7 * m + 3) % (MAX_LEN - 1) for m in range(M)])


def _two_stage(M, H, Hkv, D, mutant=None):
    """The checks of test_gpu_qknorm.py on the emulation: stage 1 (every pos = 0: the output is n) inside the float64 interval
    and v untouched; stage 2 bit-equal to the rotation of stage 1's n.  Returns (failures per check, worst err / bound)."""
    q, k, v, gq, gk = qr.kernel_case(M, H, Hkv, D)
    cos, sin = qr.rope_tables(D, MAX_LEN)
    zero = torch.zeros(M, dtype=torch.long)
    q1, k1, v1 = qr.emulate(q, k, v, gq, gk, qr.EPS, cos, sin, zero, mutant)
    out_q, r_q = qr.norm_check(q1, q, gq, qr.EPS)
    out_k, r_k = qr.norm_check(k1, k, gk, qr.EPS)
    pos = positions(M)
    q2, k2, v2 = qr.emulate(q, k, v, gq, gk, qr.EPS, cos, sin, pos, mutant)
    c, s = cos[pos][:, None], sin[pos][:, None]
    fails = {"q norm": int(out_q.sum()), "k norm": int(out_k.sum()),
             "v": int(not (qr.same_values(v1, v) and qr.same_values(v2, v))),
             "rotation": int(not (qr.same_values(q2, qr.rope_f32(q1, c, s)) and qr.same_values(k2, qr.rope_f32(k1, c, s))))}
    return fails, max(r_q, r_k)


@pytest.mark.parametrize("M,H,Hkv,D", SHAPES)
def test_f32_emulation_in_the_kernels_order_is_inside(M, H, Hkv, D):
    fails, ratio = _two_stage(M, H, Hkv, D)
    print(f"err/bound emulation qknorm {M}x{H}/{Hkv}x{D}: {ratio:.3f}")
    assert not any(fails.values()), fails
    assert 1e-3 < ratio <= 1.0


@pytest.mark.parametrize("mutant", MUTANTS)
def test_one_mistake_variants_are_outside(mutant):
    where = {"no_eps": ("q norm", "k norm"), "mean_2d": ("q norm", "k norm"), "mean_half": ("q norm", "k norm"),
             "k_with_q_gamma": ("k norm",), "gamma_by_chunk": ("q norm", "k norm"), "norm_after_rope": ("rotation",),
             "no_bf16_round": ("rotation",), "v_normed": ("v",)}[mutant]
    seen = set()
    for shape in SHAPES:        # at every shape the mistake shows, and only in the checks it concerns (a shape with one k head
        fails, _ = _two_stage(*shape, mutant=mutant)      # may hold no k row on which a dropped eps matters)
        assert any(fails[w] > 0 for w in where), (mutant, shape, fails)
        assert all(n == 0 for w, n in fails.items() if w not in where), (mutant, shape, fails)
        seen |= {w for w in where if fails[w] > 0}
    assert seen == set(where), (mutant, seen)


def test_zero_row_gives_zeros_and_the_bound_is_zero_there():
    x = torch.zeros(1, 1, 128, dtype=torch.bfloat16)
    g = torch.full((128,), 1.5)
    ref, e = qr.qknorm_ref_bound(x, g, qr.EPS)
    assert not ref.any() and not e.any() and not qr.qknorm_f32(x, g, qr.EPS).any()


# ---- configuration and host -------------------------------------------------------------------------------------------------------
def _hf(**kw):
    base = {"model_type": "qwen3", "hidden_size": 512, "num_hidden_layers": 2, "num_attention_heads": 4, "num_key_value_heads": 2,
            "head_dim": 128, "intermediate_size": 1024, "vocab_size": 259, "rms_norm_eps": 1e-6, "attention_bias": False}
    base.update(kw)
    return base


def _cfg(**kw):
    from icl_speech_text_llm_amd.runtime.config import LlamaCfg
    base = dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, ffn=1024, vocab=260, max_pos=2048, pad_id=259, lora_rank=8,
                rms_eps=1e-6, qk_norm=True)
    base.update(kw)
    return LlamaCfg(**base)


def test_config_from_hf_sets_qk_norm():
    import dataclasses
    from icl_speech_text_llm_amd.runtime import checkpoints as ck
    from icl_speech_text_llm_amd.runtime.config import LlamaCfg
    assert dataclasses.fields(LlamaCfg)[-1].name == "qk_norm" and LlamaCfg().qk_norm is False
    c = ck.llama_cfg_from_hf(_hf(), LlamaCfg())
    assert c.qk_norm and (c.n_heads, c.kv_heads, c.head_dim, c.rms_eps) == (4, 2, 128, 1e-6)
    assert not ck.llama_cfg_from_hf(_hf(model_type="llama"), LlamaCfg()).qk_norm
    assert not ck.llama_cfg_from_hf({k: v for k, v in _hf().items() if k != "model_type"}, LlamaCfg()).qk_norm
    # the real shapes load: Qwen3-1.7B / 8B / 14B
    for hidden, heads in ((2048, 16), (4096, 32), (5120, 40)):
        c = ck.llama_cfg_from_hf(_hf(hidden_size=hidden, num_attention_heads=heads, num_key_value_heads=8), LlamaCfg())
        assert c.qk_norm and c.head_dim == 128 and c.kv_heads == 8
    # Qwen3-0.6B / 4B / 32B: head_dim 128 is not hidden / heads — the pinned refusal
    for hidden, heads in ((1024, 16), (2560, 32), (5120, 64)):
        with pytest.raises(NotImplementedError):
            ck.llama_cfg_from_hf(_hf(hidden_size=hidden, num_attention_heads=heads, num_key_value_heads=8), LlamaCfg())


def test_synth_and_packing_carry_the_gains():
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.packing import pack_llama
    c = _cfg()
    sd = synth.llama_state(c, synth._Gen(5, "cpu", torch.float32, False))
    keys = [f"llama_model.model.layers.{i}.self_attn.{n}_norm.weight" for i in range(2) for n in "qk"]
    gains = [sd[k] for k in keys]
    assert all(g.shape == (128,) and g.dtype == torch.float32 for g in gains)
    assert all(0.2 < float((g - 1).std()) < 0.4 for g in gains)
    assert all(float((a - b).abs().max()) > 0.3 for i, a in enumerate(gains) for b in gains[i + 1:])     # four different draws
    w = pack_llama(sd, c, "cpu")
    for i, L in enumerate(w.layers):
        assert torch.equal(L.q_gamma, gains[2 * i]) and torch.equal(L.k_gamma, gains[2 * i + 1])
    # without qk_norm: the same draws as before for every other tensor, no gains in the packed layers
    plain = synth.llama_state(replace(c, qk_norm=False), synth._Gen(5, "cpu", torch.float32, False))
    assert set(sd) - set(plain) == set(keys)
    wp = pack_llama(plain, replace(c, qk_norm=False), "cpu")
    assert wp.layers[0].q_gamma is None and wp.layers[0].k_gamma is None
    missing = {k: v for k, v in sd.items() if k != keys[1]}
    with pytest.raises(KeyError, match="k_norm"):
        pack_llama(missing, c, "cpu")


def test_stray_norm_keys_without_qk_norm_are_a_value_error():
    from icl_speech_text_llm_amd.models.custom_salmon import CustomSALMONN
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.packing import pack_llama
    c = _cfg()
    sd = synth.llama_state(c, synth._Gen(5, "cpu", torch.float32, False))
    with pytest.raises(ValueError, match=r"layers\.0\.self_attn\.q_norm\.weight"):
        pack_llama(sd, replace(c, qk_norm=False), "cpu")
    tiny = SalmonnCfg.tiny(use_beats=False)
    m = CustomSALMONN(device="cpu", arch=replace(tiny, llama=replace(c, qk_norm=False)), llama_path="none", beats_path="")
    with pytest.raises(ValueError, match="q_norm"):            # not dropped by strict=False
        m.load_state_dict(sd, strict=False)


def test_fp8_kv_with_qk_norm_is_a_value_error_at_construction():
    from icl_speech_text_llm_amd.models.custom_qwen import CustomQwen
    from icl_speech_text_llm_amd.models.custom_salmon import CustomSALMONN
    from icl_speech_text_llm_amd.runtime.config import QwenAudioCfg, SalmonnCfg
    from icl_speech_text_llm_amd.runtime.engines import check_kv_dtype
    tiny = SalmonnCfg.tiny(use_beats=False)
    for llama in (_cfg(), _cfg(n_kv_heads=None)):              # grouped and multi-head alike
        with pytest.raises(ValueError, match="QK-norm" if llama.group == 1 else "grouped-query|QK-norm"):
            CustomSALMONN(device="cpu", arch=replace(tiny, llama=llama), llama_path="none", beats_path="", llm_kv_dtype="fp8")
    with pytest.raises(ValueError, match="QK-norm"):
        check_kv_dtype("fp8", _cfg(n_kv_heads=None))
    assert check_kv_dtype("bf16", _cfg()) == "bf16" and check_kv_dtype("fp8", _cfg(n_kv_heads=None, qk_norm=False)) == "fp8"
    q = QwenAudioCfg.tiny()
    with pytest.raises(ValueError, match="QK-norm"):
        CustomQwen(device="cpu", arch=replace(q, llm=replace(q.llm, qk_norm=True)), model_path="none", llm_kv_dtype="fp8")


def test_plugin_state_dict_round_trip_keeps_the_gains(tmp_path):
    from icl_speech_text_llm_amd.models.custom_salmon import CustomSALMONN
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    tiny = SalmonnCfg.tiny(use_beats=False)
    arch = replace(tiny, llama=_cfg())
    a = CustomSALMONN(device="cpu", arch=arch, llama_path="none", beats_path="", seed=1)
    keys = [f"salmonn.llama_model.model.layers.{i}.self_attn.{n}_norm.weight" for i in range(2) for n in "qk"]
    sd = a.state_dict()
    assert all(k in sd and sd[k].shape == (128,) for k in keys)
    a.save_checkpoint(str(tmp_path / "ck.pt"))
    saved = torch.load(str(tmp_path / "ck.pt"), map_location="cpu")["model"]
    b = CustomSALMONN(device="cpu", arch=arch, llama_path="none", beats_path="", seed=2)
    assert not torch.equal(b.state_dict()[keys[0]], sd[keys[0]])
    b.load_state_dict(saved)
    assert all(torch.equal(b.state_dict()[k], sd[k]) for k in keys)


def test_library_exports_the_symbol_at_abi_6():
    import icl_speech_text_llm_amd.runtime.binding as b
    lib = b.load_library()
    assert b.ABI_VERSION == 6 and lib.icl_abi_version() == 6
    assert hasattr(lib, "icl_qknorm_rope_kv_bf16") and "icl_qknorm_rope_kv_bf16" in b._SIGNATURES
    with pytest.raises(b.IclError):                               # the wrapper refuses CPU tensors like its neighbours
        x = torch.zeros(1, 3 * 128, dtype=torch.bfloat16)
        g = torch.ones(128)
        cs = torch.zeros(4, 64)
        z = torch.zeros(1, dtype=torch.int32)
        b.qknorm_rope_kv(x, 128, 256, g, g, 1e-6, cs, cs, z, z, None, None, 1, 1, 128, 0)

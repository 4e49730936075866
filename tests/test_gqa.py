"""CPU: grouped-query attention (GQA) in the decoder's configuration, checkpoint ingestion, synthetic weights and packing,
the FP8-KV refusal, and the oracle's GQA path against transformers' LlamaForCausalLM."""
from dataclasses import replace

import numpy as np
import pytest
import torch


def _hf(**kw):
    base = {"hidden_size": 512, "num_hidden_layers": 2, "num_attention_heads": 4, "num_key_value_heads": 2,
            "intermediate_size": 1024, "vocab_size": 259}
    base.update(kw)
    return base


def _gqa_cfg(**kw):
    from icl_speech_text_llm_amd.runtime.config import LlamaCfg
    base = dict(hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, ffn=1024, vocab=260, max_pos=2048, pad_id=259, lora_rank=8,
                lora_targets=("q_proj", "v_proj"))
    base.update(kw)
    return LlamaCfg(**base)


def test_config_loading_reads_kv_heads():
    from icl_speech_text_llm_amd.runtime import checkpoints as ck
    from icl_speech_text_llm_amd.runtime.config import LlamaCfg
    c = ck.llama_cfg_from_hf(_hf(), LlamaCfg())
    assert (c.n_heads, c.n_kv_heads, c.kv_heads, c.group, c.head_dim) == (4, 2, 2, 2, 128)
    m = ck.llama_cfg_from_hf(_hf(num_key_value_heads=4), LlamaCfg())
    assert (m.n_kv_heads, m.kv_heads, m.group) == (None, 4, 1)
    assert ck.llama_cfg_from_hf(_hf(head_dim=128), LlamaCfg()).n_kv_heads == 2      # a matching head_dim key is fine


def test_config_refusals():
    from icl_speech_text_llm_amd.runtime import checkpoints as ck
    from icl_speech_text_llm_amd.runtime.config import LlamaCfg
    with pytest.raises(NotImplementedError, match="grouped-query"):                  # head_dim 64
        ck.llama_cfg_from_hf(_hf(hidden_size=256), LlamaCfg())
    with pytest.raises(ValueError):                                                  # 4 heads / 3 KV heads
        ck.llama_cfg_from_hf(_hf(num_key_value_heads=3), LlamaCfg())
    with pytest.raises(NotImplementedError):                                         # head_dim != hidden / heads
        ck.llama_cfg_from_hf(_hf(head_dim=64), LlamaCfg())
    with pytest.raises(ValueError):                                                  # 16 query heads per K/V head
        LlamaCfg(hidden=2048, n_heads=16, n_kv_heads=1)
    with pytest.raises(NotImplementedError, match="grouped-query"):
        LlamaCfg(hidden=256, n_heads=4, n_kv_heads=2)
    with pytest.raises(ValueError):
        LlamaCfg(n_kv_heads=5)
    assert LlamaCfg(hidden=1024, n_heads=8, n_kv_heads=1).group == 8


def test_pack_llama_validates_again():
    """pack_llama checks the head counts itself: a cfg object that slipped past LlamaCfg's own check is refused there."""
    from icl_speech_text_llm_amd.runtime.packing import pack_llama
    bad = _gqa_cfg()
    object.__setattr__(bad, "n_kv_heads", 3)
    with pytest.raises(ValueError):
        pack_llama({}, bad, "cpu")
    bad64 = _gqa_cfg()
    object.__setattr__(bad64, "hidden", 256)
    with pytest.raises(NotImplementedError, match="grouped-query"):
        pack_llama({}, bad64, "cpu")


def test_default_cfg_site_shapes_unchanged():
    from icl_speech_text_llm_amd.runtime.config import LlamaCfg
    from icl_speech_text_llm_amd.runtime.engines import site_shapes
    from icl_speech_text_llm_amd.runtime.packing import llama_k_aug, qkv_offsets, qkv_width
    c = LlamaCfg()
    assert (c.kv_heads, c.group) == (32, 1)
    assert site_shapes(c, llama_k_aug(c)) == dict(qkv=(12288, 4160), o=(4096, 4096), gu=(22016, 4096), down=(4096, 11008))
    assert qkv_offsets(c) == (4096, 8192) and qkv_width(c) == 12288


def test_gqa_shapes_and_packing():
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.engines import site_shapes
    from icl_speech_text_llm_amd.runtime.packing import llama_k_aug, pack_llama, qkv_offsets, qkv_width
    c = _gqa_cfg(qkv_bias=True)
    k_aug = llama_k_aug(c)
    assert k_aug == 576
    assert site_shapes(c, k_aug)["qkv"] == (1024, k_aug)
    assert qkv_offsets(c) == (512, 768) and qkv_width(c) == 1024
    sd = synth.llama_state(c, synth._Gen(5, "cpu", torch.float32, False))
    lp = "llama_model.model.layers.1.self_attn."
    assert sd[lp + "k_proj.weight"].shape == (256, 512) and sd[lp + "v_proj.bias"].shape == (256,)
    assert sd[lp + "v_proj.lora_B.weight"].shape == (256, 8) and sd[lp + "q_proj.lora_B.weight"].shape == (512, 8)
    w = pack_llama(sd, c, "cpu")
    L = w.layers[1]
    assert L.wqkv.shape == (1024, k_aug) and L.bqkv.shape == (1024,)
    bf = lambda t: t.to(torch.bfloat16)
    assert torch.equal(L.wqkv[:512, :512], bf(sd[lp + "q_proj.weight"]))
    assert torch.equal(L.wqkv[512:768, :512], bf(sd[lp + "k_proj.weight"]))
    assert torch.equal(L.wqkv[768:, :512], bf(sd[lp + "v_proj.weight"]))
    # LoRA K-augmentation: target 0 (q) in columns 512..519 of the q rows, target 1 (v) in 520..527 of the v rows, zero elsewhere
    assert torch.equal(L.wqkv[:512, 512:520], bf(sd[lp + "q_proj.lora_B.weight"]))
    assert torch.equal(L.wqkv[768:, 520:528], bf(sd[lp + "v_proj.lora_B.weight"]))
    aug = L.wqkv[:, 512:].clone()
    aug[:512, :8] = 0
    aug[768:, 8:16] = 0
    assert not aug.any()
    assert torch.equal(L.bqkv, torch.cat([sd[lp + f"{n}_proj.bias"].float() for n in "qkv"]))
    assert w.rope_cos.shape == (2048, 64)


def test_synth_default_draws_what_it_drew():
    """n_kv_heads=None draws exactly the multi-head tensors (same shapes, same generator order)."""
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import LlamaCfg
    kw = dict(hidden=256, n_layers=2, n_heads=2, ffn=512, vocab=260, qkv_bias=True, lora_targets=("q_proj", "k_proj"))
    a = synth.llama_state(LlamaCfg(**kw), synth._Gen(3, "cpu", torch.float32, True))
    b = synth.llama_state(LlamaCfg(n_kv_heads=2, **kw), synth._Gen(3, "cpu", torch.float32, True))
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    # and what it drew before grouped-query attention existed: every attention matrix [hidden, hidden], in this order
    g = synth._Gen(3, "cpu", torch.float32, True)
    emb = g.normal(260, 256)
    assert torch.equal(emb, a["llama_model.model.embed_tokens.weight"])
    for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
        assert torch.equal(g.normal(256, 256), a[f"llama_model.model.layers.0.self_attn.{n}.weight"])
    for n in ("q_proj", "k_proj", "v_proj"):
        assert torch.equal(g.bias(256), a[f"llama_model.model.layers.0.self_attn.{n}.bias"])


def test_fp8_kv_with_gqa_is_a_value_error_at_construction():
    from icl_speech_text_llm_amd.models.custom_qwen import CustomQwen
    from icl_speech_text_llm_amd.models.custom_salmon import CustomSALMONN
    from icl_speech_text_llm_amd.runtime.config import QwenAudioCfg, SalmonnCfg
    from icl_speech_text_llm_amd.runtime.engines import check_kv_dtype
    tiny = SalmonnCfg.tiny(use_beats=False)
    arch = replace(tiny, llama=_gqa_cfg(), qformer=replace(tiny.qformer))
    with pytest.raises(ValueError, match="grouped-query"):
        CustomSALMONN(device="cpu", arch=arch, llama_path="none", beats_path="", llm_kv_dtype="fp8")
    q = QwenAudioCfg.tiny()
    qarch = replace(q, llm=replace(q.llm, hidden=512, n_heads=4, n_kv_heads=2, ffn=1024))
    with pytest.raises(ValueError, match="grouped-query"):
        CustomQwen(device="cpu", arch=qarch, model_path="none", llm_kv_dtype="fp8")
    with pytest.raises(ValueError):
        check_kv_dtype("fp8", _gqa_cfg())
    assert check_kv_dtype("bf16", _gqa_cfg()) == "bf16" and check_kv_dtype("fp8", _gqa_cfg(n_kv_heads=None)) == "fp8"
    m = CustomSALMONN(device="cpu", arch=arch, llama_path="none", beats_path="")    # bf16 cache: constructs
    assert m.cfg.llama.group == 2
    assert m.salmonn.state_dict()["llama_model.model.layers.0.self_attn.k_proj.weight"].shape == (256, 512)


def test_oracle_gqa_matches_transformers():
    """Pins the oracle's GQA path upstream: logits and 10 greedy ids of LlamaOracle(n_kv_heads=2) against transformers'
    LlamaForCausalLM(num_key_value_heads=2) on random weights (tolerance of test_llama_forward_loss_and_generate_match_hf)."""
    from transformers import LlamaConfig, LlamaForCausalLM
    from oracle import models as om
    torch.manual_seed(0)
    hf = LlamaForCausalLM(LlamaConfig(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                      intermediate_size=1024, vocab_size=260, rms_norm_eps=1e-5, max_position_embeddings=256,
                                      pad_token_id=259, bos_token_id=1, eos_token_id=2, attn_implementation="eager")).eval()
    sd = {k: v.detach().float() for k, v in hf.state_dict().items()}
    llm = om.LlamaOracle(sd, n_heads=4, rms_eps=1e-5, n_kv_heads=2)
    ids = torch.from_numpy(np.random.default_rng(4).integers(3, 259, (2, 23)))
    emb = llm.embed(ids)
    with torch.no_grad():
        want = hf(inputs_embeds=emb).logits
        gen = hf.generate(inputs_embeds=emb, attention_mask=torch.ones(2, 23, dtype=torch.long), max_new_tokens=10,
                          min_new_tokens=10, do_sample=False, pad_token_id=259)
    got, _ = llm.forward(emb)
    assert np.abs(got.numpy() - want.numpy()).max() < 2e-4
    assert llm.generate_greedy(emb, 10, eos_id=-1, pad_id=259).tolist() == gen.tolist()

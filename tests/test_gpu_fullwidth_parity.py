"""`-m gpu`: FULL-WIDTH, SHALLOW-DEPTH value parity for BASELINE.json configs 4 and 5.

tests/test_gpu_fullsize_c45.py runs the 13B and Qwen2-Audio dims through size-independent properties only; the oracle never
touched K = 5120 / 13824, 40 heads, the 156 032-row vocabulary or the QKV-bias + LoRA-q/k path at full width.  Here the
decoders keep their REAL widths and take two layers (plus, for Qwen2-Audio, one Whisper-width audio-tower layer), which the
CPU oracle finishes in seconds — every kernel selection that depends on a width (256x256 tile at K = 5120 / 13824 / 4096,
fused RoPE epilogue with 40 heads, decode tile at N = 15360 / 27648, skinny lm_head over 156 032 rows, bias in the QKV
accumulator init, LoRA augmentation on q and k) is compared value by value:

  * against `oracle` with the bf16 rounding hook (the HIP path's own rounding points) and in pure fp32;
  * the ratio criterion wherever an fp32 run exists: rel(gpu, fp32) <= 1.25 x rel(bf16 oracle, fp32);
  * all 10 greedy decisions teacher-forced along the GPU's tokens: each must be the oracle's arg-max within 2x the step's
    measured logit error;
  * on the decisive-margin weight set (runtime/synth.py) the 10 ids must EQUAL the oracle's and the designed chain.
Contracts: the reference's llama_model(...) / .generate(...) calls (models/custom_salmon.py:630-640, 704-731) and the
Qwen2-Audio forward / generate (models/custom_qwen.py:199-247)."""
from dataclasses import replace

import numpy as np
import pytest
import torch

from gpu_support import stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
NEW = 10
RATIO = 1.25


def _rel(a, b):
    a, b = a.detach().float().cpu().reshape(-1), b.detach().float().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _ids(i, n, hi=32000):
    return np.random.default_rng(99 + i).integers(3, hi, n).tolist()


def _oracle_inputs(llm, segs, speech_rows):
    """inputs_embeds [1, S, H] of one prompt (token runs through the oracle's embedding, speech runs from `speech_rows`)."""
    parts = []
    for seg in segs:
        if isinstance(seg, tuple):
            parts.append(speech_rows[seg[1]:seg[1] + seg[2]].float().cpu())
        else:
            parts.append(llm.embed(torch.tensor(seg)))
    return torch.cat(parts)[None]


def _decoder_parity(rt, make_oracle, prompts, speech, tag, bound):
    """GPU generate (10 tokens, step logits kept) vs the oracle teacher-forced along the GPU's tokens, per prompt row."""
    from oracle import models as om
    gen = rt.generate(prompts, speech, max_new_tokens=NEW, suppress_eos=True, want_step_logits=True)
    toks, steps = gen.tokens, gen.step_logits.cpu()                       # [B, 10], [10, B, V]
    flat = None if speech is None else speech.reshape(-1, speech.shape[-1])
    for b, segs in enumerate(prompts):
        tf = {}
        for name, rnd in (("bf16", "hook"), ("fp32", None)):
            llm = make_oracle(rnd)
            tf[name] = llm.teacher_forced_logits(_oracle_inputs(llm, segs, flat), toks[b:b + 1])[0]     # [10, V]
        g = steps[:, b]
        r_b, r_f, r_o = _rel(g, tf["bf16"]), _rel(g, tf["fp32"]), _rel(tf["bf16"], tf["fp32"])
        within = 0
        for t in range(NEW):
            err = float((g[t] - tf["bf16"][t]).abs().max())
            top = tf["bf16"][t].max()
            within += int(float(top - tf["bf16"][t, int(toks[b, t])]) <= 2 * err + 1e-6)
        print(f"{tag} row {b} (S={sum(len(s) if not isinstance(s, tuple) else s[2] for s in segs)}): step logits rel vs bf16 oracle "
              f"{r_b:.2e}, vs fp32 {r_f:.2e}, bf16 oracle vs fp32 {r_o:.2e} (ratio {r_f / r_o:.2f}); choices within 2x error {within}/{NEW}")
        assert r_b <= bound, (tag, b, r_b)
        assert r_f <= RATIO * r_o, (tag, b, r_f, r_o)
        assert within == NEW, (tag, b, within)


def _margin_ids(rt, make_oracle, prompts, speech, host, prefix, tag):
    from icl_speech_text_llm_amd.runtime import synth
    gen = rt.generate(prompts, speech, max_new_tokens=NEW, suppress_eos=True)
    flat = None if speech is None else speech.reshape(-1, speech.shape[-1])
    for b, segs in enumerate(prompts):
        llm = make_oracle("hook")
        tf = llm.teacher_forced_logits(_oracle_inputs(llm, segs, flat), gen.tokens[b:b + 1])[0]
        last = [s for s in segs if not isinstance(s, tuple)][-1][-1]
        chain, t = [], int(last)
        for _ in range(NEW):
            t = synth.margin_successor(host, t, prefix=prefix)
            chain.append(t)
        top2 = tf.topk(2, dim=-1).values
        print(f"{tag} margin weights row {b}: gpu {gen.tokens[b].tolist()} oracle {tf.argmax(-1).tolist()} min margin {float((top2[:, 0] - top2[:, 1]).min()):.1f}")
        assert gen.tokens[b].tolist() == tf.argmax(-1).tolist() == chain, (tag, b)


# ----------------------------------------------------------------------------------------------------------------------
# C5: Llama-2-13B width (hidden 5120, 40 heads, FFN 13824), two layers
# ----------------------------------------------------------------------------------------------------------------------
def test_c5_13b_width_two_layers_match_oracle():
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import LlamaCfg, SalmonnCfg
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime, speech_segment
    from oracle import models as om
    cfg = SalmonnCfg(llama=LlamaCfg(hidden=5120, n_layers=2, n_heads=40, ffn=13824))
    c = cfg.llama
    speech = torch.randn(2, 88, 5120, generator=torch.Generator().manual_seed(5)).cuda() * 0.02
    a, b = _ids(0, 288), _ids(1, 512)                                    # VOXCELEB (S = 376) and HVB (S = 600) prompt lengths
    prompts = [[a[:280], speech_segment(0, 88), a[280:]], [b[:504], speech_segment(88, 88), b[504:]]]
    for margin in (False, True):
        sd = synth.salmonn_state(cfg, seed=3, device="cuda", dtype=torch.bfloat16, parts=("llama",), margin=margin)
        rt = SalmonnRuntime(cfg, dict(sd), device="cuda", parts=("llama",))
        host = {k: v.float().cpu() for k, v in sd.items()}
        del sd
        lsd = {k[len("llama_model."):]: v for k, v in host.items()}

        def make_oracle(rnd, lsd=lsd, host=host):
            return om.LlamaOracle(lsd, c.n_heads, c.rms_eps, c.rope_theta, c.lora_scale,
                                  rnd=om.bf16_round_activations(host) if rnd == "hook" else None)
        if margin:
            _margin_ids(rt, make_oracle, prompts, speech, host, "llama_model.", "13B width")
        else:
            _decoder_parity(rt, make_oracle, prompts, speech, "13B width, 2 layers", bound=1e-2)     # measured 5.4e-3, ratio 1.00, 10/10
        del rt, host, lsd
        torch.cuda.empty_cache()


# ----------------------------------------------------------------------------------------------------------------------
# C4: Qwen2-Audio widths (LM 4096 / 32 heads / 11008 / V = 156032 with QKV bias and LoRA on q, k; audio tower 1280 / 20
# heads / 5120, 128 mel bins), two decoder layers + one audio-tower layer
# ----------------------------------------------------------------------------------------------------------------------
def test_c4_qwen2_audio_width_shallow_match_oracle():
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import QwenAudioCfg
    from icl_speech_text_llm_amd.runtime.qwen import QwenAudioRuntime
    from oracle import audio_frontend as af, models as om
    full = QwenAudioCfg()
    cfg = QwenAudioCfg(audio=replace(full.audio, n_layers=1), llm=replace(full.llm, n_layers=2), audio_token_id=full.audio_token_id)
    c = cfg.llm
    assert c.vocab == 156032 and c.qkv_bias and c.lora_targets == ("q_proj", "k_proj") and cfg.audio.d_model == 1280
    lens = [480000, 16000 * 12 + 5]
    wav = torch.zeros(2, 480000)
    for i, n in enumerate(lens):
        wav[i, :n] = torch.from_numpy(np.clip(np.random.default_rng(70 + i).normal(0, 0.1, n), -1, 1).astype(np.float32))
    for margin in (False, True):
        sd = synth.qwen_audio_state(cfg, seed=4, device="cuda", dtype=torch.bfloat16, margin=margin)
        rt = QwenAudioRuntime(cfg, dict(sd), device="cuda")
        host = {k: v.float().cpu() for k, v in sd.items()}
        del sd
        feats, out_lens = rt.encode_audio(raw_wav=wav, wav_lens=lens)
        feats = feats.clone()
        if not margin:      # K13 at full width: audio tower (key padding, AvgPool, ln_post) + projector
            spec = torch.stack([torch.from_numpy(af.whisper_logmel(wav[i, :n].numpy(), n_mels=128)) for i, n in enumerate(lens)])
            mel_lens = [min(3000, -(-n // 160)) for n in lens]
            ref_b, ref_lens = om.qwen_audio_features(host, spec, mel_lens, cfg.audio.n_heads, rnd=om.bf16_round_activations(host))
            ref_f, _ = om.qwen_audio_features(host, spec, mel_lens, cfg.audio.n_heads, rnd=None)
            assert out_lens == ref_lens
            for i, n in enumerate(out_lens):
                r_b, r_f, r_o = _rel(feats[i, :n], ref_b[i, :n]), _rel(feats[i, :n], ref_f[i, :n]), _rel(ref_b[i, :n], ref_f[i, :n])
                print(f"qwen audio tower width 1280, 1 layer, audio {i}: rel vs bf16 oracle {r_b:.2e}, vs fp32 {r_f:.2e}, "
                      f"bf16 oracle vs fp32 {r_o:.2e} (ratio {r_f / r_o:.2f})")
                assert r_b <= 4e-3 and r_f <= RATIO * r_o, (i, r_b, r_f, r_o)      # measured 1.9e-3 .. 2.0e-3, ratio 1.00
        rows = []
        for bi, n_aud in enumerate(out_lens):
            ids = _ids(40 + bi, 514, hi=150000)
            rows.append(ids[:506] + [cfg.audio_token_id] * n_aud + ids[506:])
        segs = rt.segments_from_ids(rows, out_lens)
        lsd = {k[len("language_model."):]: v for k, v in host.items() if k.startswith("language_model.")}

        def make_oracle(rnd, lsd=lsd, host=host):
            return om.LlamaOracle(lsd, c.n_heads, c.rms_eps, c.rope_theta, c.lora_scale,
                                  rnd=om.bf16_round_activations(host) if rnd == "hook" else None)
        if margin:
            _margin_ids(rt, make_oracle, segs, feats, host, "language_model.", "Qwen2-Audio width")
        else:
            _decoder_parity(rt, make_oracle, segs, feats, "Qwen2-Audio width, 2 layers", bound=1e-2)     # measured 4.6e-3 / 4.9e-3, ratio 1.00
        del rt, host, lsd
        torch.cuda.empty_cache()

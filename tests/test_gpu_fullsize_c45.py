"""`-m gpu`: BASELINE.json configs 4 and 5 at their FULL dims — the size-independent properties of
tests/test_gpu_fullsize.py on

  * C5: SALMONN with Llama-2-13B dims (hidden 5120, 40 layers, 40 heads, FFN 13824) over the multi-task round-robin of
    prompt lengths 376 / 600 / 408 (VOXCELEB / HVB / VOXPOPULI, 5 text exemplars + 88 audio positions);
  * C4: Qwen2-Audio at the 7B-Instruct dims (vocab 156032, QKV bias, LoRA on q/k) with one 750-row audio in a 1264-position
    prompt.

Checked: batch invariance (bit-exact: a row's arithmetic never depends on what it is packed with), causality, determinism,
HIP-graph replay == eager decode, exactly max_new_tokens ids inside the vocabulary.  The CPU oracle is too slow to be the
checker at these sizes; value parity at full size is covered on the 7B chain (test_gpu_fullsize.py) and at miniature dims
for both model families (test_gpu_models.py, test_gpu_qwen.py) — the kernels selected here (256x256 tile at K = 5120 / 13824,
fused RoPE epilogue with 40 heads, decode tile at N = 15360 / 27648, vocabulary 156032 lm_head) are the same code paths.
"""
import numpy as np
import pytest
import torch

from gpu_support import stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _wav(i, n=480000):
    return torch.from_numpy(np.clip(np.random.default_rng(1234 + i).normal(0, 0.1, n), -1, 1).astype(np.float32))


def _ids(i, n, hi=32000):
    return np.random.default_rng(99 + i).integers(3, hi, n).tolist()


# ----------------------------------------------------------------------------------------------------------------------
# C5: Llama-2-13B dims
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rt13():
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    cfg = SalmonnCfg.llama2_13b()
    sd = synth.salmonn_state(cfg, seed=0, device="cuda", dtype=torch.bfloat16)
    r = SalmonnRuntime(cfg, sd, device="cuda", consume=True)
    del sd
    yield r
    del r
    torch.cuda.empty_cache()


def _c5_prompts(speech_rows=88):
    from icl_speech_text_llm_amd.runtime.salmonn import speech_segment
    out = []
    for b, n_text in enumerate((288, 512, 320)):          # VOXCELEB / HVB / VOXPOPULI text tokens
        ids = _ids(b, n_text)
        out.append([ids[:n_text - 8], speech_segment(b * speech_rows, speech_rows), ids[n_text - 8:]])
    return out


def test_c5_13b_prefill_is_batch_invariant_and_causal(rt13):
    wav = torch.stack([_wav(i) for i in range(3)])
    speech = rt13.encode_speech(wav, [480000] * 3).clone()
    assert speech.shape == (3, 88, 5120) and torch.isfinite(speech).all()
    solo_sp = rt13.encode_speech(wav[1:2], [480000])
    assert torch.equal(solo_sp[0], speech[1])
    prompts = _c5_prompts()
    both, lens = rt13.forward_logits(prompts, speech)
    both = both.clone()
    assert lens == [376, 600, 408] and both.shape == (1384, 32001) and torch.isfinite(both).all()
    off = 0
    for b, n in enumerate(lens):
        from icl_speech_text_llm_amd.runtime.salmonn import speech_segment
        segs = [prompts[b][0], speech_segment(0, 88), prompts[b][2]]
        solo, _ = rt13.forward_logits([segs], speech[b:b + 1])
        assert torch.equal(solo, both[off:off + n]), f"row {b} (S={n}) depends on its batch neighbours"
        off += n
    # causality on the longest row: change its last 8 tokens -> all earlier positions unchanged
    from icl_speech_text_llm_amd.runtime.salmonn import speech_segment
    p = prompts[1]
    alt_tail = [(t + 7) % 31000 + 3 for t in p[2]]
    alt, _ = rt13.forward_logits([[p[0], speech_segment(0, 88), alt_tail]], speech[1:2])
    ref = both[376:976]
    assert torch.equal(alt[:592], ref[:592]) and not torch.equal(alt[592:], ref[592:])


def test_c5_13b_generate_deterministic_graph_equals_eager(rt13):
    speech = torch.randn(3, 88, 5120, device="cuda") * 0.02
    prompts = _c5_prompts()
    rt13._graphs.clear(); rt13._graph_warm.clear()
    runs = [rt13.generate(prompts, speech, max_new_tokens=10, suppress_eos=True).tokens.clone() for _ in range(3)]
    assert len(rt13._graphs) == 1                                  # eager, capture + replay, replay
    assert runs[0].shape == (3, 10) and torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert int(runs[0].min()) >= 0 and int(runs[0].max()) < 32001
    assert all(L.decode_packed is not None for L in rt13.llama.w.layers)      # the decode tile ran on decode-packed weights
    # a row generated alone gives the same first token (prefill is batch invariant; later tokens go through decode tiles
    # whose summation order depends on the batch size class, so only token 0 is required to be identical)
    from icl_speech_text_llm_amd.runtime.salmonn import speech_segment
    solo = rt13.generate([[prompts[1][0], speech_segment(0, 88), prompts[1][2]]], speech[1:2], max_new_tokens=10,
                         suppress_eos=True).tokens
    assert int(solo[0, 0]) == int(runs[0][1, 0])


# ----------------------------------------------------------------------------------------------------------------------
# C4: Qwen2-Audio at full dims
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rtq():
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import QwenAudioCfg
    from icl_speech_text_llm_amd.runtime.qwen import QwenAudioRuntime
    cfg = QwenAudioCfg()
    sd = synth.qwen_audio_state(cfg, seed=0, device="cuda", dtype=torch.bfloat16)
    r = QwenAudioRuntime(cfg, sd, device="cuda", consume=True)
    del sd
    yield r
    del r
    torch.cuda.empty_cache()


def _c4_rows(cfg, audio_rows):
    """input_ids rows in the HF layout: text, a run of <|AUDIO|> ids as long as the audio's valid feature rows, text."""
    rows = []
    for b, n_aud in enumerate(audio_rows):
        ids = _ids(40 + b, 514, hi=150000)
        rows.append(ids[:506] + [cfg.audio_token_id] * n_aud + ids[506:])
    return rows


def test_c4_qwen2_audio_full_dims_invariance_causality_generate(rtq):
    cfg = rtq.cfg
    wav = torch.zeros(2, 480000)
    lens = [480000, 16000 * 12 + 5]
    for i, n in enumerate(lens):
        wav[i, :n] = _wav(70 + i, n)
    feats, out_lens = rtq.encode_audio(raw_wav=wav, wav_lens=lens)
    feats = feats.clone()
    assert feats.shape == (2, 750, 4096) and out_lens[0] == 750 and 0 < out_lens[1] < 750
    assert torch.isfinite(feats[0]).all() and torch.isfinite(feats[1, :out_lens[1]]).all()
    solo_f, solo_l = rtq.encode_audio(raw_wav=wav[1:2], wav_lens=lens[1:])
    assert solo_l == out_lens[1:] and torch.equal(solo_f[0, :solo_l[0]], feats[1, :out_lens[1]])     # key padding: batch invariant
    rows = _c4_rows(cfg, out_lens)
    segs = rtq.segments_from_ids(rows, out_lens)
    both, plens = rtq.forward_logits(segs, feats)
    both = both.clone()
    assert plens == [514 + 750, 514 + out_lens[1]] and both.shape == (sum(plens), 156032) and torch.isfinite(both).all()
    solo, _ = rtq.forward_logits(rtq.segments_from_ids(rows[:1], out_lens[:1]), feats[:1])
    assert torch.equal(solo, both[:1264])
    # causality: perturb the last 8 text tokens of row 0
    alt_row = rows[0][:-8] + [(t + 11) % 150000 + 3 for t in rows[0][-8:]]
    alt, _ = rtq.forward_logits(rtq.segments_from_ids([alt_row], out_lens[:1]), feats[:1])
    assert torch.equal(alt[:1256], both[:1256]) and not torch.equal(alt[1256:], both[1256:1264])
    # generate: deterministic, exactly 10 ids inside the vocabulary, graph replay == eager
    rtq._graphs.clear(); rtq._graph_warm.clear()
    runs = [rtq.generate(segs, feats, max_new_tokens=10, suppress_eos=True).tokens.clone() for _ in range(3)]
    assert runs[0].shape == (2, 10) and torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert int(runs[0].min()) >= 0 and int(runs[0].max()) < 156032
    assert len(rtq._graphs) == 1

"""Every stage of the audio encoder chains on the kernels, per element against float64 (`-m gpu`; all input goes through
runtime/binding.py).  tests/encoder_stage_check.py records what each launch of LogMel, WhisperEncoderHIP, QwenAudioTowerHIP,
BeatsHIP and SpeechQFormerHIP wrote and judges it against the float64 specification of that stage (oracle/encoder_stages.py: the
model definition applied to the state dict and to the logical contents of the previous stage's ACTUAL output), with the bound
that kernel family already has — errors do not accumulate over the chain, so no tolerance is introduced here.  The reference
never sees a launch's strides, offsets or counts: the host code that places the operands is under test together with the
kernels.  tests/test_encoder_stages.py runs the same check without a GPU on an emulation of the wrappers and shows that twelve
planted host-side mistakes are rejected at the stage they are planted in.

Cases (state dicts: synth.*_state(cfg, seed=0, jitter=True); clips: noise as in test_gpu_models._wavs):
  tiny ragged    clips of 30.8 s, 0.2 s and 3 s at their own lengths: T_a = 1536 > 1500 (90 windows), one patch row (T = 8), the
                 per-clip posconv GEMMs, two Q-Former runs ([1536], [1500, 1500]) and the ragged result
  tiny padded    3 s and 5 s both run at 5 s: the batched posconv GEMM (stride_a / stride_c / stride_r), rows zeroed in place,
                 kv_lens < T
  tiny reuse     the padded batch and then the 0.2 s clip alone on the SAME runtime after the ragged case: stale rows of wh_x2,
                 be_xg and qf_cat would surface here
  tiny Qwen      mel lengths 3000, 1000, 999, 2, 1: key padding at odd and even lengths, one feature frame, pooled length 0
  real width     Whisper (d 1280, 20 heads), BEATs (d 768: 96 lanes per row and 2 rows per block in beats_posconv_pack, 48
                 channels per group) and the Q-Former (768 / 2048) at their default widths with one layer each
  log-mel        spec and xt of one launch, 80 and 128 mel bins

Worst err / bound per stage kind measured on MI355X: DESIGN.md."""
import dataclasses

import numpy as np
import pytest
import torch

import encoder_stage_check as sc
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)
from oracle import audio_frontend as af

pytestmark = pytest.mark.gpu

RAGGED = [480000 + 12345, 3200, 16000 * 3 + 123]
PADDED = [16000 * 3 + 123, 16000 * 5]
QWEN_MEL_LENS = [3000, 1000, 999, 2, 1]


def _wavs(lens, L=None, seed=1234):                     # as tests/test_gpu_models.py::_wavs
    L = L or max(lens)
    wav = torch.zeros(len(lens), L)
    for i, n in enumerate(lens):
        rng = np.random.default_rng(seed + i)
        wav[i, :n] = torch.from_numpy(np.clip(rng.normal(0, 0.1, n), -1, 1).astype(np.float32))
    return wav


def _salmonn(cfg):
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    parts = ("whisper", "beats", "qformer")
    sd = synth.salmonn_state(cfg, seed=0, jitter=True, parts=parts)
    rt = SalmonnRuntime(cfg, dict(sd), device=DEV, parts=parts)
    sc.check_packed(sd, rt)
    return cfg, sd, rt


@pytest.fixture(scope="module")
def tiny(B):
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    return _salmonn(SalmonnCfg.tiny(use_beats=True)) + ({"ragged": False},)


def _encode(env, lens, padded, case):
    cfg, sd, rt = env[:3]
    wav = _wavs(lens)
    with sc.recording() as launches:
        out = rt.encode_speech(wav, lens, padded_lens=padded).clone()
    worst = sc.walk_salmonn(launches, sd, cfg, wav, lens, padded, out)
    sc.report(case, worst)
    assert max(worst.values()) <= 1.0
    return launches


def test_tiny_ragged(tiny):
    launches = _encode(tiny, RAGGED, None, "tiny ragged")
    tiny[3]["ragged"] = True
    assert tiny[2].last_audio_windows == [90, 88, 88]
    assert len(launches) == 1 + 17 + (6 + 48 + 1 + 16) + (2 + 3 + 22 + 1) + (3 + 3 + 22 + 1)


def test_tiny_padded(tiny):
    launches = _encode(tiny, PADDED, [max(PADDED)] * 2, "tiny padded")
    assert len(launches) == 1 + 17 + 39 + 29


def test_tiny_reuse(tiny):
    """The workspace has held the ragged batch (3 clips, T up to 1536) before these two run in it."""
    if not tiny[3]["ragged"]:
        tiny[2].encode_speech(_wavs(RAGGED), RAGGED)
        tiny[3]["ragged"] = True
    _encode(tiny, PADDED, [max(PADDED)] * 2, "tiny reuse padded")
    _encode(tiny, [3200], None, "tiny reuse 0.2 s")


def test_tiny_qwen_tower(B):
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import QwenAudioCfg
    from icl_speech_text_llm_amd.runtime.qwen import QwenAudioRuntime
    cfg = QwenAudioCfg.tiny()
    sd = synth.qwen_audio_state(cfg, seed=0, jitter=True)
    rt = QwenAudioRuntime(cfg, dict(sd), device=DEV)
    sc.check_packed(sd, rt)
    wav = _wavs([min(480000, 160 * m) for m in QWEN_MEL_LENS], seed=50)
    spec = torch.stack([torch.from_numpy(af.whisper_logmel(wav[i, :160 * m].numpy(), 128)) for i, m in enumerate(QWEN_MEL_LENS)])
    with sc.recording() as launches:
        feats, lens = rt.encode_audio(input_features=spec, mel_lens=QWEN_MEL_LENS)
        feats = feats.clone()
    worst = sc.walk_qwen(launches, sd, cfg.audio.n_heads, spec.to(DEV), QWEN_MEL_LENS, (feats, lens))
    sc.report("tiny qwen", worst)
    assert lens == [750, 250, 250, 0, 0]
    assert max(worst.values()) <= 1.0


def test_real_width_one_layer(B):
    """Each engine on its own at the real widths: Whisper on one clip, BEATs on two ragged clips of 1.0 s and 2.5 s, the
    Q-Former on the Whisper rows and the second clip's BEATs rows."""
    from icl_speech_text_llm_amd.runtime.config import BeatsCfg, QFormerCfg, SalmonnCfg, WhisperCfg
    cfg, sd, rt = _salmonn(dataclasses.replace(SalmonnCfg.tiny(lora=False), whisper=WhisperCfg(n_layers=1),
                                               beats=BeatsCfg(n_layers=1), qformer=QFormerCfg(n_layers=1)))
    lens = [16000, 40000]
    wav = _wavs(lens, seed=90)
    wav_d = wav.to(DEV)
    with sc.recording() as launches:
        xt, _ = rt.logmel(rt.ws, wav_d[1:], torch.tensor(lens[1:], dtype=torch.int32, device=DEV))
    w = sc.Walk(launches, ["logmel_whisper"])
    sc.walk_logmel(w, wav[1:], lens[1:], 80)
    worst = dict(w.worst)
    with sc.recording() as launches:
        speech = rt.whisper.forward(rt.ws, xt)
    worst.update(_merge(worst, sc.check_whisper(launches, sd, cfg, xt)))
    with sc.recording() as launches:
        audio, cu, T = rt.beats.forward(rt.ws, wav_d, lens, lens)
    assert T == [48, 120]
    worst.update(_merge(worst, sc.check_beats(launches, sd, cfg, wav, lens, lens, (audio, cu, T))))
    a1, cu1 = audio[cu[1]:cu[2]], [0, T[1]]
    with sc.recording() as launches:
        out = rt.qformer.forward(rt.ws, speech, 1, a1, cu1)
    worst.update(_merge(worst, sc.check_qformer(launches, sd, cfg, speech, a1, cu1, out)))
    sc.report("real width", worst)
    assert max(worst.values()) <= 1.0


def _merge(a, b):
    return {k: max(a.get(k, 0.0), v) for k, v in b.items()}


@pytest.mark.parametrize("n_mels", [80, 128])
def test_logmel_spec_and_xt(B, n_mels):
    from icl_speech_text_llm_amd.runtime import engines as E
    lens = [16000 + 77, 200]
    wav = _wavs(lens, seed=70)
    lm, ws = E.LogMel(n_mels, DEV), E.Workspace(DEV)
    with sc.recording() as launches:
        lm(ws, wav.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), want_spec=True)
    w = sc.Walk(launches, ["logmel_whisper"])
    sc.walk_logmel(w, wav, lens, n_mels)
    w.done()
    sc.report(f"log-mel {n_mels}", w.worst)
    assert max(w.worst.values()) <= 1.0

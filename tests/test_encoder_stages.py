"""The stage check of the audio encoder chains (tests/encoder_stage_check.py) without a GPU: the engines of runtime/engines.py run
on CPU tensors with every runtime.binding wrapper they call replaced by its emulation (tests/encoder_emulation.py), which reads
and writes through the launch's own strides, offsets and counts.  The host code that places the operands is what is under test
here, in every run: each launch's output must meet the float64 specification of its stage (oracle/encoder_stages.py), which
knows nothing of the launch's arguments.

Second half: planted mistakes.  Each alters the arguments of ONE launch before the emulation sees them (all stay inside their
buffers) and must be rejected by the stage check at the stage it was planted in — this is what shows that the inputs (random
clips, lengths that are no multiple of a block) make the mistake exceed the stage's bound."""
import dataclasses

import numpy as np
import pytest
import torch

import encoder_emulation as emu
import encoder_stage_check as sc
from oracle import audio_frontend as af

RAGGED = [480000 + 12345, 3200, 16000 * 3 + 123]        # > 30 s (T_a = 1536, 90 windows), 0.2 s (one patch row), 3 s
PADDED = [16000 * 3 + 123, 16000 * 5]                   # both run at the longer length: key padding, rows zeroed in place
QWEN_MEL_LENS = [3000, 1000, 999, 2, 1]


def _wavs(lens, L=None, seed=1234):                     # as tests/test_gpu_models.py::_wavs
    L = L or max(lens)
    wav = torch.zeros(len(lens), L)
    for i, n in enumerate(lens):
        rng = np.random.default_rng(seed + i)
        wav[i, :n] = torch.from_numpy(np.clip(rng.normal(0, 0.1, n), -1, 1).astype(np.float32))
    return wav


@pytest.fixture(scope="module")
def salmonn():
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    cfg = SalmonnCfg.tiny(use_beats=True)
    sd = synth.salmonn_state(cfg, seed=0, jitter=True, parts=("whisper", "beats", "qformer"))
    rt = sc.cpu_salmonn(cfg, sd)
    sc.check_packed(sd, rt)
    return cfg, sd, rt


@pytest.fixture(scope="module")
def qwen():
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import QwenAudioCfg
    cfg = QwenAudioCfg.tiny()
    sd = synth.qwen_audio_state(cfg, seed=0, jitter=True)
    rt = sc.cpu_qwen(cfg, sd)
    sc.check_packed(sd, rt)
    return cfg, sd, rt


def _encode(env, lens, padded, case, mutate=None):
    cfg, sd, rt = env
    wav = _wavs(lens)
    with emu.installed(mutate), sc.recording() as launches:
        out = rt.encode_speech(wav, lens, padded_lens=padded).clone()
    worst = sc.walk_salmonn(launches, sd, cfg, wav, lens, padded, out)
    sc.report(case, worst)
    assert max(worst.values()) <= 1.0
    return launches


def test_salmonn_ragged_padded_reuse(salmonn):
    """The three tiny SALMONN cases on ONE runtime and workspace, in the order that makes stale buffer contents matter: the
    ragged batch (per-clip posconv GEMMs, Q-Former runs [1536] and [1500, 1500]), the padded batch (batched posconv GEMM,
    kv_lens < T), the padded batch again and the 0.2 s clip alone (wh_x2, be_xg and qf_cat hold the earlier cases' rows)."""
    rt = salmonn[2]
    launches = _encode(salmonn, RAGGED, None, "cpu ragged")
    assert rt.qformer.last_windows == [90, 88, 88]
    assert len(launches) == 1 + 17 + (6 + 48 + 1 + 16) + (2 + 3 + 22 + 1) + (3 + 3 + 22 + 1)
    launches = _encode(salmonn, PADDED, [max(PADDED)] * 2, "cpu padded")
    assert len(launches) == 1 + 17 + 39 + 29
    _encode(salmonn, PADDED, [max(PADDED)] * 2, "cpu reuse padded")
    _encode(salmonn, [3200], None, "cpu reuse 0.2 s")


def _qwen_spec(mel_lens, seed=50):
    wav = _wavs([min(480000, 160 * m) for m in mel_lens], seed=seed)
    return torch.stack([torch.from_numpy(af.whisper_logmel(wav[i, :160 * m].numpy(), 128)) for i, m in enumerate(mel_lens)])


def _tower(env, mel_lens, case, mutate=None):
    cfg, sd, rt = env
    spec = _qwen_spec(mel_lens)
    with emu.installed(mutate), sc.recording() as launches:
        feats, lens = rt.encode_audio(input_features=spec, mel_lens=mel_lens)
        feats = feats.clone()
    worst = sc.walk_qwen(launches, sd, cfg.audio.n_heads, spec, mel_lens, (feats, lens))
    sc.report(case, worst)
    assert max(worst.values()) <= 1.0
    return lens


def test_qwen_tower(qwen):
    """Key padding at odd and even lengths, one feature frame with pooled length 0, the max(1, f) clamp."""
    assert _tower(qwen, QWEN_MEL_LENS, "cpu qwen") == [750, 250, 250, 0, 0]


def test_logmel_spec_and_xt():
    """spec and xt of one launch for 80 and 128 mel bins (the engines ask for both only through log_mel())."""
    from icl_speech_text_llm_amd.runtime import engines as E
    lens = [16000 + 77, 200]
    wav = _wavs(lens, seed=70)
    for n_mels in (80, 128):
        lm, ws = E.LogMel(n_mels, "cpu"), E.Workspace("cpu")
        with emu.installed(), sc.recording() as launches:
            lm(ws, wav, torch.tensor(lens, dtype=torch.int32), want_spec=True)
        w = sc.Walk(launches, ["logmel_whisper"])
        sc.walk_logmel(w, wav, lens, n_mels)
        w.done()
        assert max(w.worst.values()) <= 1.0


def test_real_width_one_layer():
    """Whisper, BEATs and the Q-Former at their default widths, one layer each: the packed weights bit for bit, and each engine
    on its own (the case tests/test_gpu_encoder_stages.py runs on the kernels)."""
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import BeatsCfg, QFormerCfg, SalmonnCfg, WhisperCfg
    cfg = dataclasses.replace(SalmonnCfg.tiny(lora=False), whisper=WhisperCfg(n_layers=1), beats=BeatsCfg(n_layers=1),
                              qformer=QFormerCfg(n_layers=1))
    sd = synth.salmonn_state(cfg, seed=0, jitter=True, parts=("whisper", "beats", "qformer"))
    rt = sc.cpu_salmonn(cfg, sd)
    sc.check_packed(sd, rt)
    lens = [16000, 40000]
    wav = _wavs(lens, seed=90)
    with emu.installed(), sc.recording() as launches:
        xt, _ = rt.logmel(rt.ws, wav[1:], torch.tensor(lens[1:], dtype=torch.int32))
        xt = xt.clone()
    with emu.installed(), sc.recording() as launches:
        speech = rt.whisper.forward(rt.ws, xt)
    worst = [sc.check_whisper(launches, sd, cfg, xt)]
    with emu.installed(), sc.recording() as launches:
        audio, cu, T = rt.beats.forward(rt.ws, wav, lens, lens)
    assert T == [48, 120]
    worst.append(sc.check_beats(launches, sd, cfg, wav, lens, lens, (audio, cu, T)))
    a1, cu1 = audio[cu[1]:cu[2]], [0, T[1]]
    with emu.installed(), sc.recording() as launches:
        out = rt.qformer.forward(rt.ws, speech, 1, a1, cu1)
    worst.append(sc.check_qformer(launches, sd, cfg, speech, a1, cu1, out))
    assert max(max(w.values()) for w in worst) <= 1.0


def test_chain_change_is_named(salmonn):
    cfg, sd, rt = salmonn
    xt = torch.zeros(1, 3002, 128, dtype=torch.bfloat16)
    with emu.installed(), sc.recording() as launches:
        rt.whisper.forward(rt.ws, xt, final_ln=False)
    with pytest.raises(sc.ChainChanged, match="update the stage list"):
        sc.check_whisper(launches, sd, cfg, xt)


# ---------------------------------------------------------------------------------------------------------------------------
# planted mistakes: (engine, wrapper, ordinal of that wrapper's launch in the engine's forward, edit, stage that must reject it)
# ---------------------------------------------------------------------------------------------------------------------------
def _stale_x2_row0(a):
    a["a"] = a["a"].clone()                              # (a copy: the module's workspace stays clean for the other tests)
    a["a"][:, 0] = 1.0                                   # conv2's operand is the padded buffer: its row 0 must be zero


def _pos_rolled(a):
    a["residual"] = a["residual"].roll(1, 0)


def _valid_plus1(a):
    a["valid_rows"] = a["valid_rows"] + 1


def _image_row_late(a):
    a["a"] = a["a"][a["lda"]:]                           # lda = channels per group = one image row


def _no_kv_lens(a):
    a["kv_lens"] = None


def _cu_moved(a):
    cu = a["cu_rows"].clone()
    cu[1] += 8
    a["cu_rows"] = cu


def _other_gate(a):
    a["rel_gate"] = a["rel_gate"].roll(int(a["cu_seqlens"][1]), 0)


def _alpha_one(a):
    a["alpha"] = 1.0


def _cat_not_cleared(a):
    out = a["out"]                                       # clip 0's ln_audio block of cat; the rows after it, to the buffer's
    C = out.stride(0)                                    # end, were cleared just before: put a stale value back
    rows = (out.untyped_storage().nbytes() // 2 - out.storage_offset()) // C
    torch.as_strided(out, (rows - out.shape[0], out.shape[1]), (C, 1), out.storage_offset() + out.shape[0] * C).fill_(0.5)


def _window_late(a):
    a["kv"] = a["kv"][1:]


def _pair_late(a):
    x = a["x"]                                           # frames 2t -> frames 2t + 2
    a["x"] = torch.as_strided(x, x.shape, x.stride(), x.storage_offset() + x.stride(0))


def _kv_lens_plus1(a):
    a["kv_lens"] = a["kv_lens"] + 1


MUTANTS = {
    "stale_x2_row0":    ("whisper", "gemm", 1, _stale_x2_row0, "whisper.conv2"),
    "pos_rolled":       ("whisper", "gemm", 1, _pos_rolled, "whisper.conv2"),
    "valid_plus1":      ("beats", "beats_posconv_pack", 0, _valid_plus1, "beats.posconv_pack.x"),
    "image_row_late":   ("beats", "gemm", 2, _image_row_late, "beats.posconv"),
    "no_kv_lens":       ("beats", "attn_fwd", 0, _no_kv_lens, "beats.L0.attn"),
    "cu_moved":         ("beats", "beats_patchify", 0, _cu_moved, "beats.patchify"),
    "other_gate":       ("beats", "attn_fwd", 0, _other_gate, "beats.L0.attn"),
    "alpha_one":        ("beats", "layernorm", 2, _alpha_one, "beats.L0.ln1"),
    "cat_not_cleared":  ("qformer", "layernorm", 1, _cat_not_cleared, "qformer.cat"),
    "window_late":      ("qformer", "qformer_window_xattn", 0, _window_late, "qformer.L0.xattn"),
    "pair_late":        ("qwen", "axpby_cast", 1, _pair_late, "qwen.pool_even"),
    "kv_lens_plus1":    ("qwen", "attn_fwd", 0, _kv_lens_plus1, "qwen.L0.attn"),
}


def _run_engine(engine, salmonn, qwen, mutate):
    """The engine's forward on the emulation (with ``mutate``), then its stage check."""
    g = torch.Generator().manual_seed(5)
    if engine == "qwen":
        return _tower(qwen, [1000, 2, 1], "mutant", mutate)
    cfg, sd, rt = salmonn
    if engine == "whisper":
        spec = torch.randn(1, cfg.whisper.n_mels, 3000, generator=g) * 0.5
        with emu.installed():
            xt = rt.logmel.from_spectrogram(rt.ws, spec).clone()
        with emu.installed(mutate), sc.recording() as launches:
            rt.whisper.forward(rt.ws, xt)
        return sc.check_whisper(launches, sd, cfg, xt)
    if engine == "beats":
        wav, L = _wavs(PADDED), max(PADDED)
        with emu.installed(mutate), sc.recording() as launches:
            x, cu, T = rt.beats.forward(rt.ws, wav, [L, L], PADDED)
            x = x.clone()
        return sc.check_beats(launches, sd, cfg, wav, [L, L], PADDED, (x, cu, T))
    cu = [0, 152, 152 + 248]                             # BEATs tokens of a 3 s and a 5 s clip
    speech = torch.randn(2 * 1500, cfg.whisper.d_model, generator=g)
    audio = torch.randn(cu[-1], cfg.beats.d_model, generator=g)
    with emu.installed(mutate), sc.recording() as launches:
        out = rt.qformer.forward(rt.ws, speech, 2, audio, cu).clone()
    return sc.check_qformer(launches, sd, cfg, speech, audio, cu, out)


@pytest.mark.parametrize("engine", ["whisper", "beats", "qformer"])
def test_engine_alone_passes(salmonn, qwen, engine):
    """The inputs of the planted mistakes, unaltered: every stage inside its bound."""
    assert max(_run_engine(engine, salmonn, qwen, None).values()) <= 1.0


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_planted_mistake_is_rejected_at_its_stage(salmonn, qwen, name):
    engine, wrapper, ordinal, edit, stage = MUTANTS[name]
    hit = []

    def mutate(n, k, arguments):
        if n == wrapper and k == ordinal:
            hit.append(1)
            edit(arguments)

    with pytest.raises(sc.StageFailure) as info:
        _run_engine(engine, salmonn, qwen, mutate)
    assert hit == [1], "the launch the mistake is planted in did not happen"
    assert info.value.stage == stage, f"rejected at {info.value.stage}, planted at {stage}: {info.value}"
    print(f"{name}: {info.value}")

"""The audio front-ends of csrc/frontend.hip against the float64 oracle (oracle/audio_frontend.py), per element (`-m gpu`).
Both kernels compute in float64 and round at the end, so the bounds are a few f32 roundings plus a float64 slack of 2^-30
(fp64_bounds.whisper_ref_bound / kaldi_ref_bound; tests/test_glue_bounds.py shows on the CPU that a direct DFT accumulated in
f32, a symmetric window, a reflect padding off by one, a missing clamp, a recursive pre-emphasis, a plain Hann window and a
missing DC removal all leave them, and measures the slack).

Whisper: one launch per n_mel of 9 clips — lengths 0, 1, 150, 200, 201 (the reflect padding and the first window), 8000, 116807
(not a multiple of the hop), 480000 and 500000 (trimmed to 480000) — of noise, a 1 kHz tone, DC, +-1 full scale and noise at
1e-6 (every energy at the 1e-10 floor); NaN past each length; xt pitches 80, 88 and 128; spec or xt absent; icl_spec_to_xt;
and a dense filter matrix, which does not fit the kernel's LDS tap table and runs the global-memory projection.
Kaldi: lengths around 0 | 1, 1 | 2, 16 | 17 and 64 | 65 frames (the kernel's groups of 16 and blocks of 64 frames) and 48000;
max_frames below a clip's frame count.

Worst err / bound measured on MI355X (every check prints `err/bound <kernel> <case>: <worst>`); every test passes, no kernel
had to change:
  logmel_whisper   0.244 (n_mel = 128, the one-sample clip), 0.16-0.20 on the other clips and on the dense filters; 0 on the empty
                   clip and on the all-floor clip, where every output is (-10 + 4) / 4 = -1.5 exactly.
  fbank_kaldi      0.969 (full scale, 560 samples), 0.92-0.97 on every clip but DC (0.527: every output is the one value
                   (log(eps) - mean) / (2 std)); 0 on the 399-sample clip, which has no frame.  The kernel rounds once, from
                   float64, and the bound is that one rounding, U |r|, plus the 2^-30 slack: a correct kernel must come this
                   close to 1, and anything with a second f32 rounding in it does not fit.
"""
import numpy as np
import pytest
import torch

import fp64_bounds as fb
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)
from oracle import audio_frontend as af

pytestmark = pytest.mark.gpu

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
T = af.N_FRAMES

W_CLIPS = [(0, "noise"), (1, "full"), (150, "noise"), (200, "tone"), (201, "dc"), (8000, "floor"), (116807, "noise"),
           (480000, "tone"), (500000, "full")]
W_WIDTH = 500008
K_CLIPS = [(399, "noise"), (400, "dc"), (559, "tone"), (560, "full"), (400 + 160 * 15, "floor"), (400 + 160 * 16, "noise"),
           (400 + 160 * 63, "tone"), (400 + 160 * 64, "dc"), (48000, "noise")]
MEAN32, STD32 = float(np.float32(af.FBANK_MEAN)), float(np.float32(af.FBANK_STD))     # what the kernel receives


def _report(kernel, data, worst):
    print(f"err/bound {kernel} {data}: {worst:.3f}")


def _signal(kind, L, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    x = {"noise": lambda: np.clip(rng.normal(0, 0.1, L), -1, 1), "tone": lambda: 0.5 * np.sin(2 * np.pi * 1000.0 * t / 16000.0),
         "dc": lambda: np.full(L, 0.25), "full": lambda: rng.choice([-1.0, 1.0], L), "floor": lambda: rng.normal(0, 1e-6, L)}[kind]()
    return x.astype(np.float32)


def _batch(clips, width):
    """([n, width] f32 with NaN past each length, lengths): every sample the kernels may not read is NaN."""
    wav = torch.full((len(clips), width), float("nan"), dtype=F32)
    for i, (L, kind) in enumerate(clips):
        wav[i, :L] = torch.from_numpy(_signal(kind, L, 1000 + i))
    return wav, [L for L, _ in clips]


@pytest.fixture(scope="module")
def whisper_clips():
    wav, lens = _batch(W_CLIPS, W_WIDTH)
    return wav, lens, wav.to(DEV), torch.tensor(lens, dtype=I32, device=DEV)


def _whisper_refs(wav, lens, n_mel, filters=None):
    return [torch.from_numpy(af.whisper_logmel(wav[i, :L].numpy(), n_mel, filters=filters, as_f64=True)) for i, L in enumerate(lens)]


def _assert_spec(spec, refs, what):
    spec = spec.cpu()
    assert bool(torch.isfinite(spec).all())
    for i, r in enumerate(refs):
        ref, e = fb.whisper_ref_bound(r)
        worst = fb.worst_ratio(spec[i], ref, e)
        _report("logmel_whisper", f"{what} clip {W_CLIPS[i][1]} {W_CLIPS[i][0]}", worst)
        bad = ~fb.within(spec[i], ref, e)
        assert not bool(bad.any()), f"{what} clip {i}: {int(bad.sum())} outside, first at {bad.nonzero()[0].tolist()}, worst {worst}"


def _launch(B, clips, mel, n_mel, *, spec=True, xt_ld=None):
    _, _, wav_d, wl = clips
    n = wav_d.shape[0]
    s = torch.full((n, n_mel, T), float("nan"), dtype=F32, device=DEV) if spec else None
    xt = torch.full((n, T + 2, xt_ld), float("nan"), dtype=BF16, device=DEV) if xt_ld else None
    ws = torch.empty(n * n_mel * T + n, dtype=F32, device=DEV)
    B.logmel_whisper(wav_d, wl, mel, n_mel, s, xt, ws)
    return s, xt


def _xt_of(spec, xt_ld):
    n, n_mel, _ = spec.shape
    want = torch.zeros(n, T + 2, xt_ld, dtype=BF16, device=spec.device)     # zero edge rows, zero columns >= n_mel
    want[:, 1:T + 1, :n_mel] = spec.transpose(1, 2).to(BF16)
    return want


@pytest.mark.parametrize("n_mel", [80, 128])
def test_logmel_whisper(B, whisper_clips, n_mel):
    wav, lens, _, _ = whisper_clips
    mel = torch.from_numpy(af.slaney_mel_filters(n_mel)).to(DEV)
    lds = [ld for ld in (80, 88, 128) if ld >= n_mel]
    spec, xt = _launch(B, whisper_clips, mel, n_mel, xt_ld=lds[0])
    _assert_spec(spec, _whisper_refs(wav, lens, n_mel), f"n_mel={n_mel}")
    assert torch.equal(xt, _xt_of(spec, lds[0]))
    spec_only, _ = _launch(B, whisper_clips, mel, n_mel)
    assert torch.equal(spec_only, spec)
    for ld in lds:
        _, xt_only = _launch(B, whisper_clips, mel, n_mel, spec=False, xt_ld=ld)
        assert torch.equal(xt_only, _xt_of(spec, ld)), ld
        xt2 = torch.full_like(xt_only, float("nan"))
        B.spec_to_xt(spec, xt2)
        assert torch.equal(xt2, xt_only), ld


def test_logmel_whisper_dense_filters(B, whisper_clips):
    """80 x 201 non-negative taps: 16080 of them against the 640 the LDS table holds, so the projection reads global memory."""
    wav, lens, _, _ = whisper_clips
    filt = np.random.default_rng(5).random((80, 201)) * 0.02
    spec, _ = _launch(B, whisper_clips, torch.from_numpy(filt).to(DEV), 80)
    _assert_spec(spec, _whisper_refs(wav, lens, 80, filters=filt), "dense filters")


def test_fbank_kaldi(B):
    wav, lens = _batch(K_CLIPS, 48008)
    n = len(lens)
    banks = torch.from_numpy(af.kaldi_mel_banks()).to(DEV)
    max_frames = af.kaldi_num_frames(48000)
    wav_d, wl = wav.to(DEV), torch.tensor(lens, dtype=I32, device=DEV)
    out = torch.full((n, max_frames, 128), float("nan"), dtype=F32, device=DEV)
    B.fbank_kaldi(wav_d, wl, banks, max_frames, af.FBANK_MEAN, af.FBANK_STD, out)
    out = out.cpu()
    refs = []
    for i, L in enumerate(lens):
        ref, e = fb.kaldi_ref_bound(torch.from_numpy(af.kaldi_fbank(wav[i, :L].numpy(), MEAN32, STD32, as_f64=True)))
        refs.append((ref, e))
        nf = af.kaldi_num_frames(L)
        assert ref.shape[0] == nf and bool(torch.isnan(out[i, nf:]).all())          # rows >= n_frames keep the fill ...
        assert bool(torch.isfinite(out[i, :nf]).all())                               # ... and the rows below it are all written
        worst = fb.worst_ratio(out[i, :nf], ref, e) if nf else 0.0
        _report("fbank_kaldi", f"clip {K_CLIPS[i][1]} {L}", worst)
        bad = ~fb.within(out[i, :nf], ref, e)
        assert not bool(bad.any()), f"clip {i}: {int(bad.sum())} outside, first at {bad.nonzero()[0].tolist()}, worst {worst}"
    assert [af.kaldi_num_frames(L) for L in lens] == [0, 1, 1, 2, 16, 17, 64, 65, 298]
    # max_frames below the clip's 298 frames: exactly 70 rows, and what follows the tensor is not touched
    buf = torch.full((71 * 128 + 4096,), float("nan"), dtype=F32, device=DEV)
    B.fbank_kaldi(wav_d[n - 1:], wl[n - 1:], banks, 70, af.FBANK_MEAN, af.FBANK_STD, buf[:70 * 128].view(1, 70, 128))
    buf = buf.cpu()
    ref, e = refs[n - 1]
    got = buf[:70 * 128].view(70, 128)
    _report("fbank_kaldi", "max_frames=70", fb.worst_ratio(got, ref[:70], e[:70]))
    assert bool(fb.within(got, ref[:70], e[:70]).all()) and bool(torch.isnan(buf[70 * 128:]).all())

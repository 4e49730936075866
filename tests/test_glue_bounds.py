"""The glue and audio front-end bounds of tests/fp64_bounds.py, checked on the CPU without the kernels, in the manner of
test_fp64_bounds.py: a plain torch / numpy f32 emulation in each kernel's own operation order stays inside its bound at every
element with a worst err / bound above 1e-3 (the bound is not vacuous), and an implementation with one deliberate mistake leaves
it — where the mistake is local, in the affected rows or columns and nowhere else.

The front-end bounds carry a float64 slack of 2^-30: test_two_float64_formulations_agree measures the distance between the
oracle (rfft) and a direct DFT summed in reverse order and asserts it stays below 2^-30 / 8 (measured: 7.3e-12 at most)."""
import math

import numpy as np
import pytest
import torch

import fp64_bounds as fb
from oracle import audio_frontend as af

BF16, F32 = torch.bfloat16, torch.float32


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _all_inside_and_biting(ratio, what):
    print(f"err/bound emulation {what}: {ratio:.3f}")
    assert 1e-3 < ratio <= 1.0, (what, ratio)


# ---- bf16 interval ------------------------------------------------------------------------------------------------------------
def test_bf16_rne_is_the_cast_on_f32_values_and_rounds_doubles_once():
    x = torch.cat([_randn(4096, seed=1) * 3, torch.tensor([0.0, -0.0, 1.0, 2.0 ** -130, 1.00390625, 1.01171875])])
    assert torch.equal(fb.bf16_rne(x.double()), x.to(BF16).double())                   # incl. the two ties to even
    just_above_a_tie = torch.tensor([1.00390625 + 2.0 ** -40], dtype=torch.float64)    # float32 would round it onto the tie
    assert float(fb.bf16_rne(just_above_a_tie)) == 1.0078125
    lo, hi = fb.bf16_interval(torch.tensor([1.0], dtype=torch.float64), torch.tensor([1e-9], dtype=torch.float64))
    assert float(lo) == float(hi) == 1.0


# ---- RoPE -----------------------------------------------------------------------------------------------------------------------
H_R, D_R, M_R = 3, 64, 6
POS_R = [0, 5, 1, 15, 9, 2]


@pytest.fixture(scope="module")
def rope():
    x = _randn(M_R, H_R, D_R, seed=21).to(BF16)
    inv = 1.0 / (10000 ** (torch.arange(0, D_R, 2).float() / D_R))
    ang = torch.arange(17).float()[:, None] * inv[None, :]
    return x, ang.cos(), ang.sin()


def _rope_f32(x, c, s, *, trunc=False, interleaved=False):
    """rope_rot8: products and sums rounded separately in f32, then one bf16 rounding.  c / s [M, 1, D / 2]."""
    xf = x.float()
    h = xf.shape[-1] // 2
    if interleaved:
        a, b = xf[..., 0::2], xf[..., 1::2]
        v = torch.stack([a * c - b * s, b * c + a * s], -1).flatten(-2)
    else:
        a, b = xf[..., :h], xf[..., h:]
        v = torch.cat([a * c - b * s, b * c + a * s], -1)
    if trunc:
        return (v.view(torch.int32) & -65536).view(F32).to(BF16)
    return v.to(BF16)


def _rope_check(rope, got):
    x, cos, sin = rope
    p = torch.tensor(POS_R)
    ref, e = fb.rope_ref_bound(x, cos[p][:, None], sin[p][:, None])
    lo, hi = fb.bf16_interval(ref, e)
    return ~fb.in_interval(got, lo, hi), fb.interval_ratio(got, ref, lo, hi)


def test_rope_f32_is_inside(rope):
    x, cos, sin = rope
    p = torch.tensor(POS_R)
    got = _rope_f32(x, cos[p][:, None], sin[p][:, None])
    out, ratio = _rope_check(rope, got)
    assert int(out.sum()) == 0
    _all_inside_and_biting(ratio, "rope")
    assert torch.equal(got[0], x[0])                                   # position 0 is the identity


@pytest.mark.parametrize("mutant", ["sin_sign", "next_pos", "interleaved", "truncate"])
def test_rope_mutants_are_outside_in_their_row(rope, mutant):
    x, cos, sin = rope
    p = torch.tensor(POS_R)
    c, s = cos[p][:, None], sin[p][:, None]
    good = _rope_f32(x, c, s)
    row = 3
    if mutant == "sin_sign":
        bad = _rope_f32(x, c, -s)
    elif mutant == "next_pos":
        bad = _rope_f32(x, cos[p + 1][:, None], sin[p + 1][:, None])
    elif mutant == "interleaved":
        bad = _rope_f32(x, c, s, interleaved=True)
    else:
        bad = _rope_f32(x, c, s, trunc=True)
    got = good.clone()
    got[row] = bad[row]
    out, _ = _rope_check(rope, got)
    assert int(out[row].sum()) > 0
    if mutant != "truncate":              # a wrong rotation shows in most of the row (the slowest frequencies barely turn in one step)
        assert int(out[row].sum()) > 0.5 * H_R * D_R, int(out[row].sum())
    out[row] = False
    assert int(out.sum()) == 0


# ---- axpby ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", [F32, BF16])
@pytest.mark.parametrize("add_dtype", [None, F32, BF16])
@pytest.mark.parametrize("in_dtype", [F32, BF16])
@pytest.mark.parametrize("alpha", [1.0, 0.5, 0.3, -1.7])
def test_axpby_f32_fused_and_unfused_are_inside(in_dtype, add_dtype, out_dtype, alpha):
    x = _randn(13, 70, seed=31).to(in_dtype)
    add = _randn(13, 70, seed=32).to(add_dtype) if add_dtype is not None else None
    a32 = torch.tensor(alpha, dtype=F32)
    unfused = x.float() * a32
    fused = x.double() * a32.double()
    if add is not None:
        unfused = unfused + add.float()
        fused = fused + add.double()
    ref, e = fb.axpby_ref_bound(x, alpha, add)
    worst = 0.0
    for v in (unfused, fused.float()):
        got = v.to(out_dtype)
        if out_dtype == BF16:
            lo, hi = fb.bf16_interval(ref, e)
            assert bool(fb.in_interval(got, lo, hi).all())
            worst = max(worst, fb.interval_ratio(got, ref, lo, hi))
        else:
            assert bool(fb.within(got, ref, e).all())
            worst = max(worst, fb.worst_ratio(got, ref, e))
    if alpha in (0.3, -1.7):                # (a product with a power of two is exact, and so are some of those forms: err 0)
        _all_inside_and_biting(worst, f"axpby {in_dtype} {add_dtype} {out_dtype} {alpha}")


@pytest.mark.parametrize("out_dtype", [F32, BF16])
def test_axpby_alpha_after_the_add_is_outside(out_dtype):
    x, add = _randn(13, 70, seed=31), _randn(13, 70, seed=32)
    ref, e = fb.axpby_ref_bound(x, 0.3, add)
    got = ((x + add) * 0.3).to(out_dtype)
    inside = fb.in_interval(got, *fb.bf16_interval(ref, e)) if out_dtype == BF16 else fb.within(got, ref, e)
    assert int((~inside).sum()) > 0.9 * x.numel()


# ---- LoRA down ------------------------------------------------------------------------------------------------------------------
def _butterfly(v):
    """wave_reduce_sum over the last axis (64 lanes): v += v[lane ^ o], o = 32 .. 1, every lane in f32."""
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def _lora_f32(x, a, scale, *, drop_last_chunk=False, no_scale=False):
    """lora_down_kernel's order: lane l sums the 8 products at k = 8 l + 512 i .. + 7 in ascending k, then the wave tree."""
    M, K0 = x.shape
    Kp = -(-K0 // 512) * 512
    prod = torch.zeros(M, a.shape[0], Kp)
    prod[..., :K0] = x.float()[:, None, :] * a.float()[None, :, :]
    if drop_last_chunk:
        prod[..., K0 - 8:K0] = 0
    prod = prod.view(M, a.shape[0], Kp // 512, 64, 8)
    s = torch.zeros(M, a.shape[0], 64)
    for i in range(Kp // 512):
        for t in range(8):
            s = s + prod[:, :, i, :, t]
    tot = _butterfly(s)
    return (tot if no_scale else tot * torch.tensor(scale, dtype=F32)).to(BF16)


def _lora_case(r, K0, seed=41):
    return (_randn(5, K0, seed=seed) * 0.5).to(BF16), (_randn(r, K0, seed=seed + 1) * 0.05).to(BF16)


def _lora_outside(got, x, a, scale):
    ref, e = fb.lora_ref_bound(x, a, scale)
    lo, hi = fb.bf16_interval(ref, e)
    return ~fb.in_interval(got, lo, hi), fb.interval_ratio(got, ref, lo, hi)


@pytest.mark.parametrize("r,K0,scale", [(1, 8, 2.0), (3, 64, -0.5), (16, 520, 2.0), (17, 1280, -0.5), (4, 4096, 2.0)])
def test_lora_f32_is_inside(r, K0, scale):
    x, a = _lora_case(r, K0)
    out, ratio = _lora_outside(_lora_f32(x, a, scale), x, a, scale)
    assert int(out.sum()) == 0
    _all_inside_and_biting(ratio, f"lora r={r} K0={K0}")


def test_lora_mutants_are_outside():
    x, a = _lora_case(16, 520)
    out, _ = _lora_outside(_lora_f32(x, a, 2.0, drop_last_chunk=True), x, a, 2.0)
    assert int(out.sum()) > 0.5 * out.numel(), int(out.sum())            # 8 products of 520: far above the rounding of the rest
    out, _ = _lora_outside(_lora_f32(x, a, 2.0, no_scale=True), x, a, 2.0)
    assert int(out.sum()) > 0.9 * out.numel()
    got = _lora_f32(x, a, 2.0)
    got[2] = _lora_f32(x, a, 2.0, drop_last_chunk=True)[2]                # local: one row
    out, _ = _lora_outside(got, x, a, 2.0)
    assert int(out[2].sum()) > 0
    out[2] = False
    assert int(out.sum()) == 0


# ---- BEATs gate -----------------------------------------------------------------------------------------------------------------
def _gate_f32(q, w, b, a, *, swap=False, no_two=False):
    M, H, _ = q.shape
    qf = q.float()
    acc = b.expand(M, H, 8).clone()
    for d in range(64):
        acc = acc + w[:, d] * qf[..., d:d + 1]
    sa = ((acc[..., 0] + acc[..., 1]) + acc[..., 2]) + acc[..., 3]
    sb = ((acc[..., 4] + acc[..., 5]) + acc[..., 6]) + acc[..., 7]
    if swap:
        sa, sb = sb, sa
    ga, gb = 1.0 / (1.0 + torch.exp(-sa)), 1.0 / (1.0 + torch.exp(-sb))
    v = ga * (gb * a - 1.0)
    return v if no_two else v + 2.0


def _gate_case(qscale):
    q = (_randn(21, 12, 64, seed=51) * qscale).to(BF16)
    return q, _randn(8, 64, seed=52) * 0.2, _randn(8, seed=53), torch.rand(12, generator=torch.Generator().manual_seed(54)) + 0.5


@pytest.mark.parametrize("qscale", [1.0, 40.0])
def test_gate_f32_is_inside(qscale):
    q, w, b, a = _gate_case(qscale)
    ref, e = fb.gate_ref_bound(q, w, b, a)
    got = _gate_f32(q, w, b, a)
    assert bool(fb.within(got, ref, e).all()), fb.worst_ratio(got, ref, e)
    _all_inside_and_biting(fb.worst_ratio(got, ref, e), f"gate x{qscale}")
    if qscale == 40.0:                                                     # both sigmoids saturate each way
        s = torch.sigmoid((q.double() @ w.double().t() + b.double()).view(21, 12, 2, 4).sum(-1))
        assert bool((s < 1e-9).any(0).any(0).all()) and bool((s > 1 - 1e-9).any(0).any(0).all())


@pytest.mark.parametrize("qscale", [1.0, 40.0])
def test_gate_mutants_are_outside(qscale):
    q, w, b, a = _gate_case(qscale)
    ref, e = fb.gate_ref_bound(q, w, b, a)
    # (saturated, the swap shows only where the two sigmoids sit at different ends: about half of the elements)
    assert int((~fb.within(_gate_f32(q, w, b, a, swap=True), ref, e)).sum()) > 0.25 * ref.numel()
    assert int((~fb.within(_gate_f32(q, w, b, a, no_two=True), ref, e)).sum()) == ref.numel()


# ---- cross entropy --------------------------------------------------------------------------------------------------------------
def _ce_f32(logits, labels, *, no_max=False, mean_over_all=False, label_shift=0):
    """ce_rows_kernel / ce_mean_kernel in their order: thread t takes v = t, t + 256, ..; wave trees; the four wave sums."""
    M, V = logits.shape
    y = labels.long()
    valid = (y >= 0) & (y < V)
    Vp = -(-V // 256) * 256
    x = torch.full((M, Vp), -math.inf)
    x[:, :V] = logits
    mx = torch.zeros(M, 1) if no_max else x.max(-1, keepdim=True).values
    ex = torch.exp(x - mx).view(M, Vp // 256, 256)
    s = torch.zeros(M, 256)
    for i in range(Vp // 256):
        s = s + ex[:, i]
    w = _butterfly(s.view(M, 4, 64))
    tot = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    yy = torch.where(valid, (y + label_shift) % V, torch.zeros_like(y))
    rows = torch.log(tot) + mx[:, 0] - logits.gather(1, yy[:, None])[:, 0]
    rows = torch.where(valid, rows, torch.zeros(M))
    Mp = -(-M // 256) * 256
    r = torch.zeros(Mp)
    r[:M] = rows
    s = torch.zeros(256)
    for i in range(Mp // 256):
        s = s + r[i * 256:(i + 1) * 256]
    w = _butterfly(s.view(4, 64))
    S = ((w[0] + w[1]) + w[2]) + w[3]
    C = torch.tensor(float(M if mean_over_all else int(valid.sum())))
    return rows, (S / C if C > 0 else torch.tensor(math.nan))


def _ce_case(M, V, scale, seed=61):
    logits = _randn(M, V, seed=seed) * scale
    labels = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(seed + 1), dtype=torch.int32)
    labels[0], labels[1] = -100, V
    if M > 4:
        labels[2], labels[3] = V - 1, 0
    return logits, labels


def _ce_outside(rows, mean, logits, labels):
    ref, e, mref, me = fb.ce_ref_bound(logits, labels)
    out = ~fb.within(rows, ref, e)
    mean_out = not abs(float(mean) - mref) <= me
    return out, mean_out, fb.worst_ratio(rows, ref, e), abs(float(mean) - mref) / me


@pytest.mark.parametrize("M,V,scale", [(9, 200, 30.0), (9, 4099, 0.01), (5, 32001, 4.0), (300, 257, 4.0), (9, 1, 4.0)])
def test_ce_f32_is_inside(M, V, scale):
    logits, labels = _ce_case(M, V, scale)
    rows, mean = _ce_f32(logits, labels)
    out, mean_out, ratio, mratio = _ce_outside(rows, mean, logits, labels)
    assert int(out.sum()) == 0 and not mean_out, (ratio, mratio)
    if V > 1:                                                               # V = 1: every loss is exactly 0
        _all_inside_and_biting(ratio, f"ce rows M={M} V={V} x{scale}")
        _all_inside_and_biting(mratio, f"ce mean M={M} V={V} x{scale}")
    assert bool((rows[:2] == 0).all())                                      # the ignored rows


def test_ce_all_ignored_is_nan_and_zero_rows():
    logits, labels = _ce_case(9, 200, 4.0)
    labels[:] = -100
    rows, mean = _ce_f32(logits, labels)
    ref, e, mref, me = fb.ce_ref_bound(logits, labels)
    assert math.isnan(float(mean)) and math.isnan(mref) and bool((rows == 0).all()) and bool((ref == 0).all())


def test_ce_mutants_are_outside():
    logits, labels = _ce_case(9, 200, 30.0)
    rows, mean = _ce_f32(logits, labels, no_max=True)                       # exp(90) overflows: inf / NaN counts as outside
    out, mean_out, _, _ = _ce_outside(rows, mean, logits, labels)
    assert int(out.sum()) > 0 and mean_out
    logits, labels = _ce_case(9, 200, 4.0)
    rows, mean = _ce_f32(logits, labels, mean_over_all=True)                # 7 valid rows of 9
    out, mean_out, _, _ = _ce_outside(rows, mean, logits, labels)
    assert int(out.sum()) == 0 and mean_out
    rows, mean = _ce_f32(logits, labels, label_shift=1)
    out, mean_out, _, _ = _ce_outside(rows, mean, logits, labels)
    valid = (labels >= 0) & (labels < 200)
    assert bool(out[valid].all()) and not bool(out[~valid].any()) and mean_out


# ---- audio front-ends -----------------------------------------------------------------------------------------------------------
def _signals(L, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    return {"noise": np.clip(rng.normal(0, 0.1, L), -1, 1), "tone": 0.5 * np.sin(2 * np.pi * 1000.0 * t / 16000.0),
            "dc": np.full(L, 0.25), "full": rng.choice([-1.0, 1.0], L), "floor": rng.normal(0, 1e-6, L)}


def _dft_power(frames, nfft, dtype=np.float64):
    """|DFT|^2 of the rows of `frames` (zero-padded to nfft) at bins 0 .. nfft / 2, as a direct sum taken from the last sample
    to the first."""
    n = np.arange(frames.shape[1])[::-1]
    k = np.arange(nfft // 2 + 1)
    ang = 2.0 * np.pi * ((n[:, None] * k[None, :]) % nfft) / nfft
    f = np.ascontiguousarray(frames[:, ::-1]).astype(dtype)
    re, im = f @ np.cos(ang).astype(dtype), f @ np.sin(ang).astype(dtype)
    return (re * re + im * im).astype(np.float64)


def _whisper_direct(wav, n_mel=80, *, f32_dft=False, symmetric=False, reflect_shift=0, clamp=True):
    """The Whisper log-mel as the kernel orders it: float64 up to l = log10(max(mel, 1e-10)), then f32: round l, the maximum,
    - 8, the clamp, + 4, / 4.  The keywords are the mutants."""
    x = np.zeros(af.N_SAMPLES)
    w = np.asarray(wav, dtype=np.float32).astype(np.float64)[:af.N_SAMPLES]
    x[:w.shape[0]] = w
    j = np.arange(-200, af.N_SAMPLES + 200)
    j = np.where(j < 0, -j + reflect_shift, j)
    j = np.where(j >= af.N_SAMPLES, 2 * (af.N_SAMPLES - 1) - j - reflect_shift, j)
    padded = x[j]
    n = np.arange(400)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / (399.0 if symmetric else 400.0))
    frames = padded[np.arange(af.N_FRAMES)[:, None] * 160 + n[None, :]] * win[None, :]
    power = _dft_power(frames, 400, np.float32 if f32_dft else np.float64)
    mel = af.slaney_mel_filters(n_mel) @ power.T
    l64 = np.log10(np.maximum(mel, 1e-10))
    l = torch.from_numpy(l64).float()
    if clamp:
        l = torch.maximum(l, l.max() - 8.0)
    return (l + 4.0) / 4.0, torch.from_numpy((np.maximum(l64, l64.max() - 8.0) + 4.0) / 4.0)


def _kaldi_direct(wav, mean, std, *, recursive_preemph=False, povey=True, dc=True):
    x = np.asarray(wav, dtype=np.float32).astype(np.float64) * 32768.0
    nf = af.kaldi_num_frames(x.shape[0])
    fr = x[np.arange(nf)[:, None] * 160 + np.arange(400)[None, :]]
    if dc:
        fr = fr - fr.sum(axis=1, keepdims=True) / 400.0
    if recursive_preemph:
        y = fr.copy()
        for n in range(1, 400):
            y[:, n] = fr[:, n] - 0.97 * y[:, n - 1]
        y[:, 0] = fr[:, 0] - 0.97 * fr[:, 0]
        fr = y
    else:
        fr = fr - 0.97 * np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(400) / 399.0)
    fr = fr * (win ** 0.85 if povey else win)[None, :]
    mel = _dft_power(fr, 512) @ af.kaldi_mel_banks().T
    out = (np.log(np.maximum(mel, np.finfo(np.float32).eps)) - mean) / (2.0 * std)
    return torch.from_numpy(out).float(), torch.from_numpy(out)


MEAN32, STD32 = float(np.float32(af.FBANK_MEAN)), float(np.float32(af.FBANK_STD))
W_CLIPS = [("noise", 8000), ("tone", 8000), ("dc", 8000), ("full", 8000), ("floor", 8000), ("noise", 1), ("noise", 150)]
K_CLIPS = [("noise", 2000), ("tone", 2000), ("dc", 2000), ("full", 2000), ("floor", 2000), ("noise", 400)]


def test_two_float64_formulations_agree():
    worst = 0.0
    for kind, L in W_CLIPS:
        wav = _signals(L)[kind]
        _, direct = _whisper_direct(wav)
        worst = max(worst, float((direct - torch.from_numpy(af.whisper_logmel(wav, as_f64=True))).abs().max()))
    for kind, L in K_CLIPS:
        wav = _signals(L)[kind]
        _, direct = _kaldi_direct(wav, MEAN32, STD32)
        worst = max(worst, float((direct - torch.from_numpy(af.kaldi_fbank(wav, MEAN32, STD32, as_f64=True))).abs().max()))
    print(f"float64 rfft vs direct DFT: {worst:.3e}")
    assert worst < fb.F64_SLACK / 8


def test_oracle_keywords_keep_the_default():
    wav = _signals(3000)["noise"]
    r64 = af.whisper_logmel(wav, as_f64=True)
    assert r64.dtype == np.float64 and np.array_equal(r64.astype(np.float32), af.whisper_logmel(wav))
    assert np.array_equal(af.whisper_logmel(wav, filters=af.slaney_mel_filters(80)), af.whisper_logmel(wav))
    k64 = af.kaldi_fbank(wav, as_f64=True)
    assert k64.dtype == np.float64 and np.array_equal(k64.astype(np.float32), af.kaldi_fbank(wav))
    assert af.kaldi_fbank(wav[:10], as_f64=True).shape == (0, 128)


@pytest.mark.parametrize("kind,L", W_CLIPS)
def test_whisper_emulation_is_inside(kind, L):
    wav = _signals(L)[kind]
    ref, e = fb.whisper_ref_bound(torch.from_numpy(af.whisper_logmel(wav, as_f64=True)))
    got, _ = _whisper_direct(wav)
    assert bool(fb.within(got, ref, e).all()), fb.worst_ratio(got, ref, e)
    if kind == "floor":                         # every energy is below 1e-10: l = -10 and r = -1.5 everywhere, exactly
        assert bool((got == -1.5).all())
    else:
        _all_inside_and_biting(fb.worst_ratio(got, ref, e), f"whisper {kind} {L}")


@pytest.mark.parametrize("mutant", ["f32_dft", "symmetric", "reflect", "no_clamp"])
def test_whisper_mutants_are_outside(mutant):
    wav = _signals(8000)["noise"]
    wav[:400] *= 0.1                            # the clip's maximum is not in the two frames the reflect mutant changes
    ref, e = fb.whisper_ref_bound(torch.from_numpy(af.whisper_logmel(wav, as_f64=True)))
    kw = {"f32_dft": dict(f32_dft=True), "symmetric": dict(symmetric=True), "reflect": dict(reflect_shift=1),
          "no_clamp": dict(clamp=False)}[mutant]
    out = ~fb.within(_whisper_direct(wav, **kw)[0], ref, e)
    assert int(out.sum()) > 0
    if mutant == "reflect":                     # frames 0 and 1 reach into the left padding; the right one is silence here
        assert int(out[:, 2:].sum()) == 0
    if mutant == "no_clamp":                    # the silent frames, well past the signal's last window
        assert bool(out[:, 60:].all()) and int(out[:, :48].sum()) == 0


@pytest.mark.parametrize("kind,L", K_CLIPS)
def test_kaldi_emulation_is_inside(kind, L):
    wav = _signals(L)[kind]
    ref, e = fb.kaldi_ref_bound(torch.from_numpy(af.kaldi_fbank(wav, MEAN32, STD32, as_f64=True)))
    got, _ = _kaldi_direct(wav, MEAN32, STD32)
    assert bool(fb.within(got, ref, e).all()), fb.worst_ratio(got, ref, e)
    _all_inside_and_biting(fb.worst_ratio(got, ref, e), f"kaldi {kind} {L}")


@pytest.mark.parametrize("mutant", ["recursive_preemph", "no_povey", "no_dc"])
def test_kaldi_mutants_are_outside(mutant):
    wav = _signals(2000)["noise"] + 0.05
    ref, e = fb.kaldi_ref_bound(torch.from_numpy(af.kaldi_fbank(wav, MEAN32, STD32, as_f64=True)))
    kw = {"recursive_preemph": dict(recursive_preemph=True), "no_povey": dict(povey=False), "no_dc": dict(dc=False)}[mutant]
    out = ~fb.within(_kaldi_direct(wav, MEAN32, STD32, **kw)[0], ref, e)
    assert int(out.sum()) > 0.5 * out.numel(), int(out.sum())

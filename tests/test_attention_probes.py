"""The attention probes of oracle/attention.py, judged without a GPU: deliberately wrong float64 references (mutants), rounded to
bf16, go through the assertion helpers tests/test_gpu_attention_exact.py applies to the kernels' output.  A mutant must be
rejected in every sequence in which its rounded output differs from the rounded true reference at all, and — so that "differs"
is not left to the mutant — in every sequence in which its definition says it must differ (``_must_differ``).  The unmutated
reference passes everything, including the weight >= 1 - 2^-12 condition on every exact row, for every shape list, head count
and form the GPU test launches: this is what fixes oracle.attention.SEED.
"""
import itertools

import pytest
import torch

from oracle import attention as oa

FORMS = list(itertools.product((64, 128), (False, True), (False, True), (False, True)))     # D, causal, kv_lens, bias
SPAN = 8              # the bias probe's rel_span: >= 8 and below every length but the shortest, so the clamp is live


def _lens(D, bias):
    return list(oa.PREFILL_LENS) + ([513] if D == 64 and not bias else [])


def _bf16(x):
    return x.to(torch.bfloat16)


def _seqs(R, mask):
    return set(R.seq[mask.flatten(1).any(1)].tolist())


def _must_differ(mut, L, kvl, causal, span_live):
    """Sequences (length L, kv_len kvl) in which the mutant is certain to change some probe's output (a safe subset)."""
    return {"drop_last": L >= 1, "dup_last": L >= 2 and kvl >= 2, "admit_next": causal and kvl >= 2, "kvlen_plus1": kvl < L,
            "shift_v": L >= 2, "swap_tiles": L >= 65, "rel_flip": L >= 8 and kvl >= 8,
            "no_clamp": span_live and L >= 32 and kvl >= 32}[mut]


def _judge(probes, mutants, must):
    """probes: name -> (ref_fn(mutate) -> Ref, fails_fn(got, R_true) -> [R, H] mask).  must: mutant -> set of sequences."""
    true = {name: ref(None) for name, (ref, _) in probes.items()}
    for name, (_, fails) in probes.items():
        R = true[name]
        assert not bool(fails(_bf16(R.ref), R).any()), f"{name}: the unmutated reference is rejected"
    for mut in mutants:
        rejected = set()
        for name, (ref, fails) in probes.items():
            R, M = true[name], ref(mut)
            got = _bf16(M.ref)
            differs = _seqs(R, (got != _bf16(R.ref)) | ~torch.isfinite(got))
            caught = _seqs(R, fails(got, R))
            assert differs <= caught, f"{mut} / {name}: differs but passes in sequences {sorted(differs - caught)}"
            rejected |= caught
        assert must[mut] <= rejected, f"{mut}: not rejected in sequences {sorted(must[mut] - rejected)}"


@pytest.mark.parametrize("D,causal,kvl,bias", FORMS)
def test_prefill_mutants_are_rejected_at_every_length(D, causal, kvl, bias):
    H, lens = (3 if D == 64 else 4), _lens(D, bias)
    kv_lens = oa.kv_lens_of(lens) if kvl else None
    kvs = [min(k, L) for k, L in zip(kv_lens or lens, lens)]
    scale, kw = D ** -0.5, dict(causal=causal, kv_lens=kv_lens)
    qc, kc, vc = oa.probe_count(lens, H, D)
    qp, kp, vp = oa.probe_peak(lens, H, D, causal=causal, kv_lens=kv_lens, head_offset=H - 3)
    qr, kr, vr = oa.random_data(lens, H, D)
    r_P = oa.R_P[f"prefill{D}"]
    probes = {
        "count": (lambda m: oa.prefill_ref(qc, kc, vc, lens, H, D, scale, mutate=m, **kw), oa.fails_count),
        "peak": (lambda m: oa.prefill_ref(qp, kp, vp, lens, H, D, scale, mutate=m, **kw), oa.fails_exact),
        "random": (lambda m: oa.prefill_ref(qr, kr, vr, lens, H, D, scale, mutate=m, **kw),
                   lambda got, R: oa.fails_bound(got, R, D, r_P)[0]),
    }
    mutants = ["drop_last", "dup_last", "shift_v", "swap_tiles", "kvlen_plus1"] + (["admit_next"] if causal else [])
    if bias:
        qb, kb, vb, table, gate = oa.probe_bias(lens, H, D, SPAN)
        rows, rest = oa.bias_exact_rows(lens, H, causal, kv_lens)
        assert rest == sum(L - (k if causal else max(k - 3, 0)) for L, k in zip(lens, kvs))
        bkw = dict(rel_bias=table, rel_gate=gate, rel_span=SPAN, **kw)

        def bias_fails(got, R):
            return oa.fails_exact(got, R, rows) | (oa.fails_bound(got, R, D, r_P)[0] & ~rows)
        probes["bias"] = (lambda m: oa.prefill_ref(qb, kb, vb, lens, H, D, scale, mutate=m, **bkw), bias_fails)
        # the other probes run with a random table under the same clamp
        g = torch.Generator().manual_seed(oa.SEED)
        rt, rg = torch.randn(H, 2 * SPAN - 1, generator=g), torch.rand(sum(lens), H, generator=g) * 2
        probes["random"] = (lambda m: oa.prefill_ref(qr, kr, vr, lens, H, D, scale, mutate=m, rel_bias=rt, rel_gate=rg, rel_span=SPAN, **kw),
                            probes["random"][1])
        mutants += ["rel_flip", "no_clamp"]
    must = {m: {s for s, (L, k) in enumerate(zip(lens, kvs)) if L and _must_differ(m, L, k, causal, True)} for m in mutants}
    _judge(probes, mutants, must)


@pytest.mark.parametrize("D,causal,kvl,bias", FORMS)
@pytest.mark.parametrize("H", [3, 4])
def test_prefill_reference_meets_every_exact_row_condition(D, causal, kvl, bias, H):
    """Both head counts of the GPU test (the mutant test above runs one): no exact row fails the condition, for the peak probe
    and for both spans of the bias probe; the number of bias rows left to the bound is the one the mask predicts."""
    lens = _lens(D, bias)
    kv_lens = oa.kv_lens_of(lens) if kvl else None
    q, k, v = oa.probe_peak(lens, H, D, causal=causal, kv_lens=kv_lens, head_offset=H - 3)
    R = oa.prefill_ref(q, k, v, lens, H, D, D ** -0.5, causal=causal, kv_lens=kv_lens)
    assert not bool(oa.fails_exact(_bf16(R.ref), R).any())
    for span in ((SPAN, 400) if bias else ()):
        q, k, v, table, gate = oa.probe_bias(lens, H, D, span)
        R = oa.prefill_ref(q, k, v, lens, H, D, D ** -0.5, causal=causal, kv_lens=kv_lens, rel_bias=table, rel_gate=gate, rel_span=span)
        rows, rest = oa.bias_exact_rows(lens, H, causal, kv_lens)
        assert not bool(oa.fails_exact(_bf16(R.ref), R, rows).any())
        assert int((~rows[:, 0]).sum()) == rest


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,reps", [(4, 1), (24, 2)])
def test_decode_mutants_are_rejected_at_every_length(D, H, reps):
    lens, max_len, scale = list(oa.DECODE_LENS) * reps, 320, D ** -0.5
    probes = {}
    for name, (q, k, v) in {"count": oa.probe_count(lens, H, D), "peak": oa.probe_peak(lens, H, D, causal=True, head_offset=reps - 1),
                            "random": oa.random_data(lens, H, D)}.items():
        kc, vc = oa.to_cache(k, v, lens, H, D, max_len, fill=1.0)
        ql = oa.last_rows(q, lens)
        fails = {"count": oa.fails_count, "peak": oa.fails_exact, "random": lambda got, R: oa.fails_bound(got, R, D, 0.0)[0]}[name]
        probes[name] = ((lambda m, ql=ql, kc=kc, vc=vc: oa.decode_ref(ql, kc, vc, lens, H, D, scale, mutate=m)), fails)
    mutants = ["drop_last", "dup_last", "shift_v", "swap_tiles", "kvlen_plus1"]
    must = {m: {s for s, L in enumerate(lens) if _must_differ(m, L, L, False, False) or (m == "kvlen_plus1" and L < max_len)}
            for m in mutants}
    if reps == 2:
        mutants = mutants[:2]          # the second launch shape differs only in the kernel's unroll: same references
    _judge(probes, mutants, must)


@pytest.mark.parametrize("win", [1, 17, 64])
def test_qformer_mutants_are_rejected(win):
    n_audio, wpa, H = 3, 3, 3
    rpa, n_win = wpa * win + 5, n_audio * wpa
    lens = [win] * n_win
    probes = {}
    for name, (q, k, v) in {"count": oa.probe_count(lens, H, 64), "peak": oa.probe_peak(lens, H, 64, causal=True),
                            "random": oa.random_data(lens, H, 64)}.items():
        kv, v_off = oa.to_windows(k, v, n_audio, wpa, win, rpa, H)
        ql = oa.last_rows(q, lens)
        fails = {"count": oa.fails_count, "peak": oa.fails_exact, "random": lambda got, R: oa.fails_bound(got, R, 64, 0.0)[0]}[name]
        probes[name] = ((lambda m, ql=ql, kv=kv, v_off=v_off: oa.qformer_ref(ql, kv, v_off, n_audio, wpa, win, rpa, H, 0.125, mutate=m)),
                        fails)
    mutants = ["drop_last", "dup_last", "shift_v"]
    must = {m: {w for w in range(n_win) if _must_differ(m, win, win, False, False)} for m in mutants}
    _judge(probes, mutants, must)


def test_offset_data_sits_near_minus_300():
    for D in (64, 128):
        q, k, _ = oa.random_data([40], 2, D, offset=True)
        s = torch.einsum("ihd,jhd->hij", q.double().view(40, 2, D), k.double().view(40, 2, D)) * D ** -0.5
        assert -310 < float(s.min()) and float(s.max()) < -285

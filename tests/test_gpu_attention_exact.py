"""Every attention kernel against the float64 reference of oracle/attention.py, per element, and with probes for which one wrong
key is far above rounding (`-m gpu`; every call goes through runtime/binding.py).  tests/test_attention_probes.py shows, without a
GPU, that the assertions used here reject a reference that drops, duplicates, admits or misplaces a single key.

The random-data bound, per element, no global tolerance (u = 2^-24, n = visible keys, A = sum_j p_j |v_j|,
S = max_j (scale * sum_i |q_i| |k_ji| + |bias_ij|)):

    |got - ref| <= ulp_bf16(max(|ref|, |got|)) + A * (r_P + c1 * D * u * S + c2 * (n + 8) * u)

Derivation.  The kernels compute o = sum_j e_j v_j / sum_j e_j with e_j = exp2(s_j - m) in f32.  (1) A score is an f32 dot product
of D exact bf16 products: |ds_j| <= C_DOT * D * u * (scale * sum_i |q_i| |k_ji| + |bias|) <= C_DOT * D * u * S with C_DOT = 2 (the
constant of test_gpu_decode_plan.py; the scaling by scale * log2(e) and the bias FMA are within it).  A weight p_j = e_j / sum e is a
ratio in which a common shift cancels, so to first order |dp_j| / p_j <= |ds_j| + max_k |ds_k| <= 2 * C_DOT * D * u * S = c1 * D * u * S,
c1 = 4, and |sum_j dp_j v_j| <= c1 * D * u * S * A.  (2) The hardware exponential is good to one ulp, the running-maximum rescales
multiply by exponentials of the same kind, the sums over n keys of e_j and of e_j v_j are f32 accumulations (C_DOT * n * u relative to
sum e_j |v_j|) and one division ends it: c2 * (n + 8) * u * A with c2 = C_DOT = 2.  (3) r_P is the kernel's own rounding of P before
the PV product, relative to each p_j and so to A: 2^-9 for the D = 64 prefill kernels (P is one bf16 term; the causal ones, which
split P, are held to the same figure), 2^-16 for D = 128 prefill (hi + lo bf16 split), 0 for decode and the Q-Former kernel (f32 throughout).  (4) The output is rounded to bf16 once: half an
ulp, taken as one ulp of the larger of |ref| and |got| so that a value next to a binade edge is not judged by the smaller spacing.
The bound is derived, not tuned: the largest err / bound per kernel is printed and recorded in DESIGN.md.

Measured on MI355X: every count, peak and bias probe passes on every kernel and form; decode, Q-Former, D = 128 prefill and the
suffix form peak at err / bound 0.48-0.49 (the output rounding alone), D = 64 prefill without a causal mask at 0.64-0.90.
What the bound found: the D = 64 CAUSAL forms, which rounded P to one bf16 term like the other D = 64 kernels, sat at 1.08 (no bias,
H = 3: sequence of 128, position 2, 3 visible keys), 1.03 (H = 4: position 5, 6 keys) and 1.04 (bias, H = 3: position 4, 5 keys).
A causal query near the start of its sequence sees a handful of keys, so two or three roundings of P near the worst case of
round-to-nearest (2^-8, twice r_P) line up with nothing to average them out; rows with >= 31 keys stay below 0.9.  Those forms
(no model runs them: every decoder here has head_dim 128) now take the two-term split of P that D = 128 has — D = 64 causal
without bias runs attn_fwd_kernel<64, true, false> in place of the interleaved kernel — and sit at 0.39-0.40.

Which test reaches which instantiation (each with a count probe and a peak probe, H = 3 and H = 4: with 128- or 256-query blocks
one grid is a multiple of 8 workgroups and the other is not, the r8 branch of the XCD remap):
  test_prefill[D=64, no bias, causal 0]              attn_fwd_il64_kernel                       (+ a 513-key sequence: third q-block)
  test_prefill[D=64, no bias, causal 1]              attn_fwd_kernel<64, true, false>           (+ a 513-key sequence: fifth q-block)
  test_prefill[D=64, bias, causal 0|1]               attn_fwd_kernel<64, false|true, true>      (BEATs: kv_lens + bias)
  test_prefill[D=128, bias 0|1, causal 0|1]          attn_fwd_kernel<128, false|true, false|true>
  ... each with kv_lens none | given, packed rows and the cache layout (NaN past each length)
  test_suffix                                        attn_fwd_kernel<128, true, false, true>
  test_prefill_unaligned_out                         the 8-byte store path of store_output (O not 16-byte aligned): il64, <128, true, false>, suffix
  test_decode[attn_decode, D, few|many]              attn_decode_kernel<D, 16|4, false, false, 8, 1>
  test_decode[attn_decode_bf16_epl16, D, few|many]   attn_decode_kernel<D, 8|4, false, false, 16, 1>   (anchors the fp8 kernels, tied to it bit for bit)
  test_decode[attn_decode_rope, D, few|many]         attn_decode_kernel<D, 16|4, true, false, 8, 1>    (target = the appended position)
  (the sixth argument is the query heads per K/V head: 2..8 are tests/test_gpu_gqa.py::test_decode_gqa)
  test_qformer[win]                                  qformer_xattn_kernel
"""
import itertools

import pytest
import torch

from gpu_support import DEV, B, dev, stop_after_a_device_fault  # noqa: F401  (fixtures)
from oracle import attention as oa

pytestmark = pytest.mark.gpu

SPAN = 8                  # rel_span of the bias probe: the clamp is live in every sequence longer than 8
FORMS = list(itertools.product((64, 128), (False, True), (False, True), (False, True)))     # D, causal, kv_lens, bias


def _report(kernel, data, worst):
    print(f"err/bound {kernel} {data}: {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------
# prefill
# ------------------------------------------------------------------------------------------------------------------
def _fwd(B, q, k, v, lens, H, D, *, cache=False, **kw):
    """One icl_attn_fwd_bf16 launch on packed rows, or with K / V in the cache layout (NaN in the rows past each length)."""
    out = torch.full((sum(lens), H * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    cu = torch.tensor(oa.cu_of(lens), dtype=torch.int32, device=DEV)
    if cache:
        k, v = oa.to_cache(k, v, lens, H, D, max(lens))
        kw["kv_cache_max_len"] = max(lens)
    B.attn_fwd(q, k, v, out, cu, max(lens), H, D, D ** -0.5, **kw)
    return out.view(-1, H, D)


@pytest.mark.parametrize("H", [3, 4])
@pytest.mark.parametrize("D,causal,kvl,bias", FORMS)
def test_prefill(B, D, causal, kvl, bias, H):
    lens = list(oa.PREFILL_LENS) + ([513] if D == 64 and not bias else [])
    total, scale, r_P = sum(lens), D ** -0.5, oa.R_P[f"prefill{D}"]
    kv_lens = oa.kv_lens_of(lens) if kvl else None
    kw = dict(causal=causal)
    if kvl:
        kw["kv_lens"] = torch.tensor(kv_lens, dtype=torch.int32, device=DEV)
    rkw = dict(causal=causal, kv_lens=kv_lens)
    g = torch.Generator().manual_seed(oa.SEED)
    span = SPAN if H == 3 else 400                                    # H = 4: rel_span larger than every length
    gate = (torch.rand(total, H, generator=g) * 2).to(DEV)
    zero = dict(rel_bias=torch.zeros(H, 2 * span - 1, device=DEV), rel_gate=gate, rel_span=span) if bias else {}
    name = f"attn_fwd D={D} causal={int(causal)} kv_lens={int(kvl)} bias={int(bias)} H={H}"

    # count and peak probes (the bias forms run them with a zero table: the weights must not move), packed and cache layout
    q, k, v = dev(*oa.probe_count(lens, H, D))
    R = oa.prefill_ref(q, k, v, lens, H, D, scale, **rkw)
    for cache in (False, True):
        oa.assert_count(_fwd(B, q, k, v, lens, H, D, cache=cache, **kw, **zero), R, f"{name} cache={int(cache)}")
    q, k, v = dev(*oa.probe_peak(lens, H, D, causal=causal, kv_lens=kv_lens, head_offset=H - 3))
    R = oa.prefill_ref(q, k, v, lens, H, D, scale, **rkw)
    for cache in (False, True):
        oa.assert_exact(_fwd(B, q, k, v, lens, H, D, cache=cache, **kw, **zero), R, None, f"{name} cache={int(cache)}")

    # random data against the bound: i.i.d. normal, and every score near -300
    rnd = dict(rel_bias=torch.randn(H, 2 * span - 1, generator=g).to(DEV), rel_gate=gate, rel_span=span) if bias else {}
    over = []
    for data in ("normal", "offset"):
        q, k, v = dev(*oa.random_data(lens, H, D, offset=data == "offset"))
        R = oa.prefill_ref(q, k, v, lens, H, D, scale, **rkw, **rnd)
        out = _fwd(B, q, k, v, lens, H, D, **kw, **rnd)
        bad, worst = oa.fails_bound(out, R, D, r_P)                      # asserted at the end: the checks below still run
        _report(name, data, worst)
        if bool(bad.any()):
            over.append(f"{name} {data}: err/bound {worst:.3g} > 1 at {oa.describe(R, bad)}")
        assert torch.equal(_fwd(B, q, k, v, lens, H, D, cache=True, **kw, **rnd), out), f"{name}: cache layout != packed rows"
        if kvl and data == "normal":
            # rows in [kv_len, len) are masked: large finite values there give the bits that zeros give
            qs, ks, vs = q.clone(), k.clone(), v.clone()
            dead = torch.cat([torch.arange(L) >= min(kv, L) for L, kv in zip(lens, kv_lens)]).to(DEV)
            ks[dead], vs[dead] = 0, 0
            assert torch.equal(_fwd(B, q, ks, vs, lens, H, D, **kw, **rnd), out), f"{name}: zeros past kv_len change the output"
            ks[dead], vs[dead] = 1e30, -1e30
            assert torch.equal(_fwd(B, q, ks, vs, lens, H, D, **kw, **rnd), out), f"{name}: 1e30 past kv_len changes the output"
            if H == 3 and not bias:
                vs[dead] = float("nan")     # the contract of icl_hip.h (rows in [kv_len, len) finite), observed, not asserted
                nan_rows = int(torch.isnan(_fwd(B, q, ks, vs, lens, H, D, **kw).float()).any(-1).any(-1).sum())
                print(f"{name}: NaN V rows in [kv_len, len) -> {nan_rows} of {total} output rows NaN")

    if bias:
        q, k, v, table, bgate = dev(*oa.probe_bias(lens, H, D, span))
        bkw = dict(rel_bias=table, rel_gate=bgate, rel_span=span)
        R = oa.prefill_ref(q, k, v, lens, H, D, scale, **rkw, **bkw)
        rows, rest = oa.bias_exact_rows(lens, H, causal, kv_lens)
        rows = rows.to(DEV)
        assert int((~rows[:, 0]).sum()) == rest == sum(L - (min(kv, L) if causal else max(min(kv, L) - 3, 0))
                                                        for L, kv in zip(lens, kv_lens or lens))
        for cache in (False, True):
            out = _fwd(B, q, k, v, lens, H, D, cache=cache, **kw, **bkw)
            oa.assert_exact(out, R, rows, f"{name} bias probe cache={int(cache)}")
            keep = torch.nonzero(~rows[:, 0])[:, 0]
            if keep.numel():
                oa.assert_bound(out[keep], R.rows(keep), D, r_P, f"{name} bias probe, rows without key i + 3")
    assert not over, "; ".join(over)


@pytest.mark.parametrize("H", [3, 4])
def test_suffix(B, H):
    """icl_attn_fwd_suffix_bf16 with q_len in {0, 1, 33, len}: the full launch's rows bit for bit, and the probes on its own output."""
    D, lens = 128, list(oa.PREFILL_LENS)
    cu, scale = oa.cu_of(lens), D ** -0.5
    qlens = [min(L, (0, 1, 33, L)[s % 4]) for s, L in enumerate(lens)]
    assert {0, 1, 33} <= set(qlens) and any(ql == L > 33 for ql, L in zip(qlens, lens))
    idx = torch.cat([torch.arange(cu[s + 1] - ql, cu[s + 1]) for s, ql in enumerate(qlens)]).to(DEV)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    cu_q = torch.tensor(oa.cu_of(qlens), dtype=torch.int32, device=DEV)

    def suffix(q, k, v):
        out = torch.full((sum(qlens), H * D), float("nan"), dtype=torch.bfloat16, device=DEV)
        B.attn_fwd(q[idx].contiguous(), k, v, out, cu_t, max(lens), H, D, scale, causal=True, cu_q=cu_q)
        return out.view(-1, H, D)

    q, k, v = dev(*oa.probe_count(lens, H, D))
    oa.assert_count(suffix(q, k, v), oa.prefill_ref(q, k, v, lens, H, D, scale, causal=True).rows(idx), "suffix")
    q, k, v = dev(*oa.probe_peak(lens, H, D, causal=True, head_offset=H - 3))
    oa.assert_exact(suffix(q, k, v), oa.prefill_ref(q, k, v, lens, H, D, scale, causal=True).rows(idx), None, "suffix")
    for data in ("normal", "offset"):
        q, k, v = dev(*oa.random_data(lens, H, D, offset=data == "offset"))
        out = suffix(q, k, v)
        R = oa.prefill_ref(q, k, v, lens, H, D, scale, causal=True).rows(idx)
        _report(f"attn_fwd_suffix H={H}", data, oa.assert_bound(out, R, D, oa.R_P["prefill128"], f"suffix {data}"))
        assert torch.equal(out, _fwd(B, q, k, v, lens, H, D, causal=True)[idx])


def test_prefill_unaligned_out(B):
    """O only 8-byte aligned (a column slice, at column 4, of a NaN-filled [rows, H * D + 12] buffer: ldo * 2 = 8 mod 16): the
    kernels leave the 16-byte row stores for the 8-byte fallback epilogue.  Same bits as the aligned launch, nothing outside O."""
    H, lens = 3, list(oa.PREFILL_LENS)
    cu = oa.cu_of(lens)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    qlens = [min(L, (0, 1, 33, L)[s % 4]) for s, L in enumerate(lens)]          # those of test_suffix
    idx = torch.cat([torch.arange(cu[s + 1] - ql, cu[s + 1]) for s, ql in enumerate(qlens)]).to(DEV)
    cu_q = torch.tensor(oa.cu_of(qlens), dtype=torch.int32, device=DEV)
    for D, causal, sfx in ((64, False, False), (128, True, False), (128, True, True)):
        q, k, v = dev(*oa.random_data(lens, H, D))
        rows, hd = (sum(qlens), H * D) if sfx else (sum(lens), H * D)
        kw = dict(causal=causal, cu_q=cu_q) if sfx else dict(causal=causal)
        if sfx:
            q = q[idx].contiguous()
        name = f"attn_fwd D={D} causal={int(causal)} suffix={int(sfx)}"
        want = torch.full((rows, hd), float("nan"), dtype=torch.bfloat16, device=DEV)
        B.attn_fwd(q, k, v, want, cu_t, max(lens), H, D, D ** -0.5, **kw)
        assert not bool(torch.isnan(want.float()).any()), name
        buf = torch.full((rows, hd + 12), float("nan"), dtype=torch.bfloat16, device=DEV)
        out = buf[:, 4:4 + hd]
        assert out.stride(0) % 4 == 0 and out.data_ptr() % 16 == 8 and out.stride(0) * 2 % 16 == 8
        B.attn_fwd(q, k, v, out, cu_t, max(lens), H, D, D ** -0.5, **kw)
        assert torch.equal(out, want), f"{name}: 8-byte-aligned O != 16-byte-aligned O"
        assert bool(torch.isnan(buf[:, :4].float()).all()) and bool(torch.isnan(buf[:, 4 + hd:].float()).all()), f"{name}: wrote outside O"


# ------------------------------------------------------------------------------------------------------------------
# decode
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,reps", [(4, 1), (24, 2)], ids=["few", "many"])     # n_seqs * H = 88 (deep unroll) | 1056 (unroll 4)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kernel", ["attn_decode", "attn_decode_bf16_epl16", "attn_decode_rope"])
def test_decode(B, kernel, D, H, reps):
    lens, max_len, scale, hd = list(oa.DECODE_LENS) * reps, 320, D ** -0.5, H * D
    n = len(lens)
    assert (n * H <= 1024) == (reps == 1)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    name = f"{kernel} D={D} {n}x{H}"

    def run(q, k, v):
        """q: the packed row of each sequence's last position.  O (and Q) are column slices of wider buffers.  attn_decode_rope gets
        the last position's raw q | k | v row (identity rotation), a cache whose row len - 1 still holds NaN, and must serve that
        position from registers and append it."""
        kc, vc = oa.to_cache(k, v, lens, H, D, max_len)
        obuf = torch.full((n, hd + 24), float("nan"), dtype=torch.bfloat16, device=DEV)
        out = obuf[:, 8:8 + hd]
        ql, kl, vl = (oa.last_rows(x, lens) for x in (q, k, v))
        if kernel == "attn_decode_rope":
            want_k, want_v = kc.clone(), vc.clone()
            pos = lens_t - 1
            kc[torch.arange(n, device=DEV), :, pos.long()] = float("nan")
            vc[torch.arange(n, device=DEV), :, pos.long()] = float("nan")
            qkv = torch.cat([ql, torch.zeros(n, 32, dtype=ql.dtype, device=DEV), kl, vl, torch.zeros(n, 32, dtype=ql.dtype, device=DEV)], 1)
            cos, sin = torch.ones(max_len, D // 2, device=DEV), torch.zeros(max_len, D // 2, device=DEV)
            B.attn_decode_rope(qkv, hd + 32, 2 * hd + 32, cos, sin, pos, None, kc, vc, out, lens_t, H, D, max_len, scale)
            assert torch.equal(kc.view(torch.int16), want_k.view(torch.int16)) and torch.equal(vc.view(torch.int16), want_v.view(torch.int16)), \
                f"{name}: the appended cache rows"
        else:
            qbuf = torch.zeros(n, hd + 64, dtype=torch.bfloat16, device=DEV)
            qbuf[:, 32:32 + hd] = ql
            getattr(B, kernel)(qbuf[:, 32:32 + hd], kc, vc, out, lens_t, H, D, max_len, scale)
        assert bool(torch.isnan(obuf[:, :8].float()).all()) and bool(torch.isnan(obuf[:, 8 + hd:].float()).all()), f"{name}: wrote outside O"
        return out.reshape(n, H, D), oa.decode_ref(ql, kc, vc, lens, H, D, scale)

    out, R = run(*dev(*oa.probe_count(lens, H, D)))
    oa.assert_count(out, R, name)
    out, R = run(*dev(*oa.probe_peak(lens, H, D, causal=True, head_offset=reps - 1)))
    oa.assert_exact(out, R, None, name)
    if reps == 1:
        assert bool((R.tgt[:, 0] == torch.tensor(lens, device=DEV) - 1).all())     # head 0: the target is the appended position
    for data in ("normal", "offset"):
        out, R = run(*dev(*oa.random_data(lens, H, D, offset=data == "offset")))
        _report(name, data, oa.assert_bound(out, R, D, oa.R_P["decode"], f"{name} {data}"))


# ------------------------------------------------------------------------------------------------------------------
# Q-Former windows
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", [1, 17, 64])
def test_qformer(B, win):
    n_audio, wpa, H = 3, 3, 3                       # 27 (window, head) pairs: not a multiple of the 4 a workgroup takes
    rpa, n_win, hd = wpa * win + 5, n_audio * wpa, H * 64     # rows_per_audio > win_per_audio * win; the rows between hold NaN
    lens = [win] * n_win

    def run(q, k, v):
        kv, v_off = oa.to_windows(k, v, n_audio, wpa, win, rpa, H)
        ql = oa.last_rows(q, lens).contiguous()
        out = torch.full((n_win, hd), float("nan"), dtype=torch.bfloat16, device=DEV)
        B.qformer_window_xattn(ql, kv, v_off, out, n_audio, wpa, win, rpa, H, 0.125)
        return out.view(n_win, H, 64), oa.qformer_ref(ql, kv, v_off, n_audio, wpa, win, rpa, H, 0.125)

    out, R = run(*dev(*oa.probe_count(lens, H, 64)))
    oa.assert_count(out, R, f"qformer win={win}")
    out, R = run(*dev(*oa.probe_peak(lens, H, 64, causal=True)))
    oa.assert_exact(out, R, None, f"qformer win={win}")
    for data in ("normal", "offset"):
        out, R = run(*dev(*oa.random_data(lens, H, 64, offset=data == "offset")))
        _report(f"qformer_window_xattn win={win}", data, oa.assert_bound(out, R, 64, oa.R_P["qformer"], f"qformer win={win} {data}"))

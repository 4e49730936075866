"""The glue kernels of csrc/elementwise.hip and rope_kv_kernel (csrc/rope_kv.hip) against float64, per element, at the shapes where
their loops and launches change
(`-m gpu`; every call goes through runtime/binding.py).  The bounds are the helpers of tests/fp64_bounds.py — each derived in
its docstring, none fitted — and tests/test_glue_bounds.py shows on the CPU that an f32 emulation in the kernel's order passes
them and that a kernel with one mistake does not.  bf16 outputs are judged by the interval check: out must lie in
[bf16(ref - e), bf16(ref + e)].  Copies, the argmax and everything a kernel must leave alone are compared bit for bit.

  test_rope_kv          rope_kv_kernel: a second pass of the two-item loop (40 heads), v_items < rope_items (GQA), D = 16 / 64 / 80
                        / 128, gaps between q | k | v, untouched cache slots, kcache = vcache = None
  test_embed_gather     embed_gather_kernel: one and several passes of both copy loops (H = 8 .. 5120), last vocab / speech rows
  test_argmax_eos       argmax_eos_kernel: V below a wave, at and past a block, +inf in the row pitch, ties across lanes / waves /
                        iterations, signed zeros, -inf, NaN; the token and finished bookkeeping
  test_axpby_cast       all 12 dtype forms x alpha 1, 0.5, 0.3, -1.7, one block and the grid-stride loop, the three source views
                        the runtime uses (row stride 0, half-row views, add aliasing out)
  test_lora_down        lora_down_kernel: r = 1 .. 64, K0 = 8 .. 4096 (ragged 512-wide steps), lda > K0, negative scale
  test_beats_gate       beats_gate_kernel: fewer threads than a block, a ragged last block, saturated sigmoids
  test_cross_entropy    ce_rows_kernel / ce_mean_kernel: V = 1 .. 32001, ignore_index and labels >= V, all rows ignored, M > 256

Worst err / bound measured on MI355X (every check prints `err/bound <kernel> <case>: <worst>`); every test passes, no kernel
had to change:
  rope_kv, axpby_cast (bf16 out), lora_down   1.000   An interval check reads 1 whenever an output equals an end of its interval,
                        and an interval is one to three bf16 values wide: the figure says "inside", not how far.  What keeps these
                        honest is the width — e is a few f32 ulps, 2^-16 of a bf16 ulp — so the interval is the RNE rounding of
                        ref and, where ref is within e of a tie, its neighbour; a truncating store is outside (CPU twin).
  axpby_cast (f32 out)  0.997 (bf16 in, f32 add, alpha = 0.5, 1030 x 1021); 0.93-0.97 without add at alpha = 0.3 and -1.7, 0 at
                        alpha = 1 and 0.5 (exact).  The bound is one rounding per operation the kernel performs, U each, so a
                        correct kernel reaches it among a million elements; there is nothing left to take off.
  beats_gate            0.108 (q x 40, saturated); 0.001 at M = H = 1, a single output whose 70-term sums happened to round well
                        (the same bound sits at 0.03-0.1 on the larger cases, and the swapped-group and missing + 2 mutants
                        leave it on the CPU).
  cross_entropy rows    0.762 (V = 200, logits x 30), 0.1-0.5 elsewhere; 0 at V = 1, where every loss is exactly 0.
  cross_entropy mean    0.089 (M = 300, V = 257).
Rows at position 0, products with alpha = 1 and ignored cross-entropy rows have bound 0 or an exact result: err 0, ratio 0.
"""
import math

import numpy as np
import pytest
import torch

import fp64_bounds as fb
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


def _report(kernel, data, worst):
    print(f"err/bound {kernel} {data}: {worst:.3f}")


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _assert_interval(out, ref, e, kernel, case):
    """bf16 `out` (CPU) inside [bf16(ref - e), bf16(ref + e)] at every element."""
    lo, hi = fb.bf16_interval(ref, e)
    worst = fb.interval_ratio(out, ref, lo, hi)
    _report(kernel, case, worst)
    bad = ~fb.in_interval(out, lo, hi)
    assert not bool(bad.any()), f"{kernel} {case}: {int(bad.sum())} outside, first at {bad.nonzero()[0].tolist()}, worst {worst}"


def _assert_within(out, ref, e, kernel, case):
    worst = fb.worst_ratio(out, ref, e)
    _report(kernel, case, worst)
    bad = ~fb.within(out, ref, e)
    assert not bool(bad.any()), f"{kernel} {case}: {int(bad.sum())} outside, first at {bad.nonzero()[0].tolist()}, worst {worst}"


# ------------------------------------------------------------------------------------------------------------------
# RoPE + KV append
# ------------------------------------------------------------------------------------------------------------------
MAX_LEN, NSEQ, SENT = 16, 3, 123.0
ROPE_ROWS = {1: [([0], [1]), ([MAX_LEN - 1], [2])],
             7: [([5, 0, MAX_LEN - 1, 3, MAX_LEN - 1, 0, 9], [0, 1, 2, 2, 0, 2, 1])]}


@pytest.mark.parametrize("M", [1, 7])
@pytest.mark.parametrize("H,Hkv,D", [(40, 40, 128), (32, 8, 128), (28, 4, 128), (14, 2, 64), (2, 2, 64), (5, 5, 80), (3, 1, 16)])
def test_rope_kv(B, H, Hkv, D, M):
    k_off = H * D + 8
    v_off = k_off + Hkv * D + 8
    ld = v_off + Hkv * D + 8                                  # = q + k + v + 24: 8-column gaps before k, before v and at the end
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D))
    ang = torch.arange(MAX_LEN).float()[:, None] * inv[None, :]
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    for case, (pos, sid) in enumerate(ROPE_ROWS[M]):
        assert len(set(zip(sid, pos))) == M
        orig = _randn(M, ld, seed=100 + H + D + case).to(BF16)
        for g0 in (H * D, k_off + Hkv * D, v_off + Hkv * D):
            orig[:, g0:g0 + 8] = SENT
        p = torch.tensor(pos)
        c, s = cos[p][:, None], sin[p][:, None]
        qkv = orig.to(DEV)
        kc = torch.full((NSEQ, Hkv, MAX_LEN, D), SENT, dtype=BF16, device=DEV)
        vc = torch.full_like(kc, SENT)
        args = (k_off, v_off, cos.to(DEV), sin.to(DEV), p.to(DEV, I32), torch.tensor(sid, dtype=I32, device=DEV))
        tail = (H, D, MAX_LEN) if H == Hkv else (H, Hkv, D, MAX_LEN)
        fn = B.rope_kv if H == Hkv else B.rope_kv_gqa
        fn(qkv, *args, kc, vc, *tail)
        got, kc, vc = qkv.cpu(), kc.cpu(), vc.cpu()
        name = f"H={H} Hkv={Hkv} D={D} M={M} pos0={pos[0]}"
        for what, off, n in (("q", 0, H), ("k", k_off, Hkv)):
            x = orig[:, off:off + n * D].view(M, n, D)
            ref, e = fb.rope_ref_bound(x, c, s)
            o = got[:, off:off + n * D].view(M, n, D)
            _assert_interval(o, ref, e, "rope_kv", f"{what} {name}")
            for m in range(M):
                if pos[m] == 0:
                    assert torch.equal(o[m], x[m]), f"{what}: a position-0 row moved"
        # everything that is not q or k holds what it held: the gaps and the v block
        keep = torch.ones(ld, dtype=torch.bool)
        keep[:H * D] = False
        keep[k_off:k_off + Hkv * D] = False
        assert torch.equal(got[:, keep], orig[:, keep])
        # the cache: the rotated k and the raw v of each row at (seq, :, pos), bit for bit; the sentinel everywhere else
        want_k, want_v = torch.full_like(kc, SENT), torch.full_like(vc, SENT)
        for m in range(M):
            want_k[sid[m], :, pos[m]] = got[m, k_off:k_off + Hkv * D].view(Hkv, D)
            want_v[sid[m], :, pos[m]] = orig[m, v_off:v_off + Hkv * D].view(Hkv, D)
        assert torch.equal(kc, want_k) and torch.equal(vc, want_v)
        # without caches: the same q and k, nothing else
        qkv2 = orig.to(DEV)
        fn(qkv2, *args[:-1], None, None, None, *tail)
        assert torch.equal(qkv2.cpu(), got)


# ------------------------------------------------------------------------------------------------------------------
# embedding gather / interleave
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ["text", "speech", "mixed"])
@pytest.mark.parametrize("H", [8, 1032, 4096, 5120])
def test_embed_gather(B, H, rows):
    V, S = 50, 6
    table = _randn(V, H, seed=H).to(BF16)
    speech = _randn(S, H, seed=H + 1)
    idx = {"text": [0, V - 1, 7], "speech": [-1, -S, -3], "mixed": [V - 1, -S, 0, -1, 5, -2]}[rows]
    out = torch.full((len(idx), H), float("nan"), dtype=F32, device=DEV)
    B.embed_gather_interleave(torch.tensor(idx, dtype=I32, device=DEV), table.to(DEV), speech.to(DEV), out)
    ref = torch.stack([table[i].float() if i >= 0 else speech[-i - 1] for i in idx])
    assert torch.equal(out.cpu(), ref)


# ------------------------------------------------------------------------------------------------------------------
# greedy argmax + EOS bookkeeping
# ------------------------------------------------------------------------------------------------------------------
def _argmax_rows(V):
    """Rows [n, V] f32 with their properties spelled out in the comments; every tie pair that fits V is used."""
    g = np.random.default_rng(V)
    rows = []

    def base():
        return g.normal(0, 1, V).astype(np.float32)

    r = base()
    r[g.integers(0, V)] = 9.0                      # a single maximum
    rows.append(r)
    r = base()
    r[V - 1] = 9.0                                 # the maximum in the last column (+inf follows in the row pitch)
    rows.append(r)
    for i, j in ((3, 10), (70, 200), (5, 256), (130, 131 + 256), (2, V - 1), (V - 2, V - 1)):
        if 0 <= i < j < V:                         # ties: two lanes; two waves; one thread, two passes; a later pass; at V - 1
            r = base()
            r[i] = r[j] = 9.0
            rows.append(r)
    r = np.full(V, -1.0, np.float32)               # +0.0 / -0.0 compare equal: the lowest index wins, whatever its sign
    r[V // 3], r[V - 1] = -0.0, 0.0
    rows.append(r)
    r = np.full(V, -1.0, np.float32)
    r[V // 3], r[V - 1] = 0.0, -0.0
    rows.append(r)
    rows.append(np.full(V, -np.inf, np.float32))   # all -inf: index 0
    rows.append(np.full(V, np.nan, np.float32))    # all NaN: index 0 (the kernel keeps a valid id)
    r = base()                                     # NaN is ignored: at index 0, next to the maximum, in the last column
    r[0] = np.nan
    if V > 3:
        r[V // 2] = 9.0
        r[V // 2 - 1] = r[V - 1] = np.nan
    rows.append(r)
    return np.stack(rows)


def _np_argmax(x):
    """The lowest index among the maxima, NaN ignored (an all-NaN row gives 0)."""
    return np.argmax(np.where(np.isnan(x), -np.inf, x), axis=1)


@pytest.mark.parametrize("V", [1, 40, 256, 257, 32001])
def test_argmax_eos(B, V):
    rows = _argmax_rows(V)
    n = rows.shape[0]
    want = _np_argmax(rows)
    buf = torch.full((n, V + 7), float("inf"), dtype=F32)
    buf[:, :V] = torch.from_numpy(rows)
    logits = buf.to(DEV)[:, :V]
    stride, pad = 6, 77777
    fin0 = np.zeros(n, np.int32)
    fin0[1::3] = 1                                                     # every third row is finished already
    e1, e2 = int(want[0]), int(want[n - 1])
    for eos, pad_id, step in ((e1, pad, 0), ((e1, e2), pad, stride - 1), (e1, e1, 2), ((e2, e1), e2, 3)):
        ids = set(eos) if isinstance(eos, tuple) else {eos}
        fin = torch.from_numpy(fin0).to(DEV)
        toks = torch.full((n, stride), -5, dtype=I32, device=DEV)
        nxt = torch.full((n,), -5, dtype=I32, device=DEV)
        B.argmax_eos(logits, eos, pad_id, fin, toks, step, nxt)
        tok = np.where(fin0 != 0, pad_id, want)
        fin_want = ((fin0 != 0) | np.isin(tok, list(ids))).astype(np.int32)
        toks = toks.cpu().numpy()
        assert toks[:, step].tolist() == tok.tolist(), (V, eos, pad_id, step)
        assert nxt.cpu().tolist() == tok.tolist()
        assert fin.cpu().tolist() == fin_want.tolist()
        toks[:, step] = -5
        assert (toks == -5).all()                                       # the other columns of out_tokens
    assert V == 1 or len(set(want.tolist())) > 2


# ------------------------------------------------------------------------------------------------------------------
# axpby / cast
# ------------------------------------------------------------------------------------------------------------------
ALPHAS = (1.0, 0.5, 0.3, -1.7)
GUARD = -77.0


def _axpby_check(B, x, add, out_dtype, alpha, case, *, add_is_out=False):
    """One launch on x [M, N] (any row stride) into the first N columns of a wider, sentinel-filled out."""
    M, N = x.shape
    wide = torch.full((M, N + 8), GUARD, dtype=out_dtype, device=DEV)
    out = wide[:, :N]
    if add_is_out:
        out.copy_(add)
        add_d = out
    else:
        add_d = add.to(DEV) if add is not None else None
    if add is not None:
        add = out.cpu().clone() if add_is_out else add
    B.axpby_cast(x.to(DEV) if not x.is_cuda else x, out, alpha=alpha, add=add_d)
    ref, e = fb.axpby_ref_bound(x.cpu(), alpha, add)
    got = wide.cpu()
    (_assert_interval if out_dtype == BF16 else _assert_within)(got[:, :N], ref, e, "axpby_cast", case)
    assert bool((got[:, N:] == GUARD).all())


@pytest.mark.parametrize("M,N", [(13, 70), (1030, 1021)])                # one partly filled block; 1030 * 1021 > 4096 * 256
@pytest.mark.parametrize("out_dtype", [F32, BF16])
@pytest.mark.parametrize("add_dtype", [None, F32, BF16])
@pytest.mark.parametrize("in_dtype", [F32, BF16])
def test_axpby_cast(B, in_dtype, add_dtype, out_dtype, M, N):
    x = _randn(M, N, seed=M).to(in_dtype)
    add = _randn(M, N, seed=M + 1).to(add_dtype) if add_dtype is not None else None
    for alpha in ALPHAS:
        _axpby_check(B, x, add, out_dtype, alpha, f"{in_dtype} {add_dtype} {out_dtype} {M}x{N} alpha={alpha}")


@pytest.mark.parametrize("alpha", ALPHAS)
def test_axpby_cast_source_views(B, alpha):
    """The three ways the runtime calls it: a row-stride-0 source (the Q-Former query broadcast to every window), the two
    half-row views of a [P, 2 d] tensor, and add aliasing out (the pooling of frames 2t and 2t + 1)."""
    W, hq = 37, 72
    q0 = _randn(1, hq, seed=7).to(DEV)
    for out_dtype in (F32, BF16):
        _axpby_check(B, q0.expand(W, hq), None, out_dtype, alpha, f"stride-0 {out_dtype} alpha={alpha}")
    P, d = 29, 40
    h = _randn(2 * P, d, seed=8).to(DEV)
    even, odd = h.view(P, 2 * d)[:, :d], h.view(P, 2 * d)[:, d:]
    assert even.stride(0) == 2 * d and torch.equal(even, h[0::2]) and torch.equal(odd, h[1::2])
    _axpby_check(B, odd, None, F32, alpha, f"odd half rows alpha={alpha}")
    first = (odd.cpu().double() * fb.f32_scalar(alpha)).float()
    _axpby_check(B, even, first, F32, alpha, f"even half rows, add is out, alpha={alpha}", add_is_out=True)
    _axpby_check(B, even, first.to(BF16), BF16, alpha, f"even half rows, add is out, bf16, alpha={alpha}", add_is_out=True)


# ------------------------------------------------------------------------------------------------------------------
# LoRA down-projection
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [2.0, -0.5])
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("r,K0", [(1, 8), (3, 64), (16, 520), (17, 1280), (21, 512), (64, 4096)])
def test_lora_down(B, r, K0, M, scale):
    lda, ldx = K0 + 8, K0 + 64 + 8
    x = (_randn(M, ldx, seed=K0 + r) * 0.5).to(BF16)
    a = (_randn(r, lda, seed=K0 + r + 1) * 0.05).to(BF16)
    xd = x.to(DEV)
    B.lora_down(xd, K0, a.to(DEV)[:, :K0], r, scale)
    got = xd.cpu()
    ref, e = fb.lora_ref_bound(x[:, :K0], a[:, :K0], scale)
    _assert_interval(got[:, K0:K0 + r], ref, e, "lora_down", f"r={r} K0={K0} M={M} scale={scale}")
    assert torch.equal(got[:, :K0], x[:, :K0]) and torch.equal(got[:, K0 + r:], x[:, K0 + r:])


# ------------------------------------------------------------------------------------------------------------------
# BEATs gate
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,H,qscale", [(1, 1, 1.0), (1, 12, 1.0), (21, 12, 1.0), (50, 12, 1.0), (300, 16, 1.0), (21, 12, 40.0)])
def test_beats_gate(B, M, H, qscale):
    ld = 3 * H * 64 + 8
    qkv = (_randn(M, ld, seed=M + H) * qscale).to(BF16)
    w, b = _randn(8, 64, seed=52) * 0.2, _randn(8, seed=53)
    a = torch.rand(H, generator=torch.Generator().manual_seed(54)) + 0.5
    gate = torch.full((M * H + 64,), float("nan"), dtype=F32, device=DEV)
    B.beats_gate(qkv.to(DEV), w.to(DEV), b.to(DEV), a.to(DEV), gate, H)
    q = qkv[:, :H * 64].view(M, H, 64)
    ref, e = fb.gate_ref_bound(q, w, b, a)
    got = gate.cpu()
    _assert_within(got[:M * H].view(M, H), ref, e, "beats_gate", f"M={M} H={H} q x{qscale}")
    assert bool(torch.isnan(got[M * H:]).all())
    if qscale != 1.0:                                                      # both sigmoids saturate each way
        s = torch.sigmoid((q.double() @ w.double().t() + b.double()).view(M, H, 2, 4).sum(-1)).view(-1, 2)
        assert bool((s < 1e-9).any(0).all()) and bool((s > 1 - 1e-9).any(0).all())


# ------------------------------------------------------------------------------------------------------------------
# cross entropy
# ------------------------------------------------------------------------------------------------------------------
def _ce_launch(B, logits, labels):
    M, V = logits.shape
    buf = torch.full((M, V + 5), float("inf"), dtype=F32)
    buf[:, :V] = logits
    rows = torch.full((M + 8,), float("nan"), dtype=F32, device=DEV)
    mean = torch.full((9,), float("nan"), dtype=F32, device=DEV)
    B.cross_entropy(buf.to(DEV)[:, :V], labels.to(DEV), rows[:M], mean[:1])
    rows, mean = rows.cpu(), mean.cpu()
    assert bool(torch.isnan(rows[M:]).all()) and bool(torch.isnan(mean[1:]).all())
    return rows[:M], float(mean[0])


@pytest.mark.parametrize("scale", [0.01, 4.0, 30.0])
@pytest.mark.parametrize("M,V", [(9, 1), (9, 200), (9, 4099), (300, 257), (5, 32001)])
def test_cross_entropy(B, M, V, scale):
    logits = _randn(M, V, seed=M + V) * scale
    labels = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(V), dtype=I32)
    labels[0], labels[1], labels[2], labels[3] = -100, V, V - 1, 0
    case = f"M={M} V={V} x{scale}"
    rows, mean = _ce_launch(B, logits, labels)
    ref, e, mref, me = fb.ce_ref_bound(logits, labels)
    _assert_within(rows, ref, e, "cross_entropy rows", case)
    assert bool((rows[:2] == 0).all())
    _report("cross_entropy mean", case, abs(mean - mref) / me if me > 0 else 0.0)
    assert abs(mean - mref) <= me, (mean, mref, me)
    # exactly one valid row: the mean is that row
    one = torch.full((M,), -100, dtype=I32)
    one[M - 2] = labels[M - 2]
    rows1, mean1 = _ce_launch(B, logits, one)
    ref1, e1, mref1, me1 = fb.ce_ref_bound(logits, one)
    _assert_within(rows1, ref1, e1, "cross_entropy rows", case + " one valid row")
    assert abs(mean1 - mref1) <= me1 and int((rows1 != 0).sum()) <= 1
    # every row ignored (-100 and >= V): zero rows and a NaN mean
    none = torch.full((M,), -100, dtype=I32)
    none[1::2] = V + 3
    rows0, mean0 = _ce_launch(B, logits, none)
    assert bool((rows0 == 0).all()) and math.isnan(mean0) and math.isnan(fb.ce_ref_bound(logits, none)[2])

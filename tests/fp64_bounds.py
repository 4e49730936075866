"""Per-element error bounds against float64, shared by test_gpu_prefill_gemm.py, test_gpu_norm_exact.py and (on the CPU, without
the kernels) test_fp64_bounds.py.  Not a test module and not a conftest: plain functions over torch tensors on any device.
The constants and the comparison of every such test live here (u = 2^-24, C_DOT = 2, bf16_ulp, assert_within, _dot).

GEMM  (pre = a @ W^T + bias in float64, mag = |a| @ |W|^T, K the depth; every bound is for the kernel's f32 value)
  e_pre                = C_DOT K u mag + u |pre| + 2u |bias|
  plain / residual     = C_DOT K u mag + u |ref| + 2u (|bias| + |residual|),  ref = pre (+ residual)
  GELU (+ residual)    = 1.13 e_pre + 1.5e-6 + u |ref| (+ 2u |residual|),     ref = gelu(pre) (+ residual)
                         1.13 >= sup |gelu'|; 1.5e-6 is the absolute-error contract of gelu_erf2 (csrc/common.h)
  SwiGLU               = 1.1 e_g (|up| + e_u) + |silu(g)| e_u + u (16 + 4 |g|) |ref|,  e_g / e_u the e_pre of gate / up
  bf16 output          = the f32 bound + 1 bf16 ulp of max(|ref|, |out|)

Norms: norm_bound() below, derived in the docstring of test_gpu_norm_exact.py.

Glue and audio front-end kernels (test_gpu_glue_exact.py, test_gpu_frontend_exact.py; on the CPU test_glue_bounds.py): the
helpers of the last section, each with its derivation in its docstring.  Their bf16 outputs are judged by bf16_interval(): out
must lie in [bf16(ref - e), bf16(ref + e)], which leaves a truncating or doubly rounding store no output ulp to hide in.

Sampling and beam-step kernels (test_gpu_decode_tail_exact.py; on the CPU test_decode_tail_bounds.py): the references and the
derivations of their bounds are in oracle/decode_tail.py; check_sampler_row() / check_beam_row() at the end judge one row."""
import math

import torch

U = 2.0 ** -24
C_DOT = 2
GELU_SLOPE = 1.13       # sup |gelu'(x)| = 1.1290
GELU_ABS = 1.5e-6       # csrc/common.h: |gelu_erf2 - exact| <= 1.5e-6 absolute
SILU_SLOPE = 1.1        # sup |silu'(x)| = 1.0998


def bf16_ulp(x):
    """Spacing of bf16 numbers at |x| (float64; subnormals counted at the smallest normal)."""
    m = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(m)) - 7)


def _dot(a, w64, w64abs):
    a64 = a.double()
    return a64 @ w64.t(), a64.abs() @ w64abs.t()


def assert_within(got, ref, bound, what):
    bad = ~((got.double() - ref).abs() <= bound)      # NaN (an element never written) counts as outside
    if bad.any():
        r, c = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, first at "
                             f"[{r}, {c}]: got {float(got[r, c])} ref {float(ref[r, c])} bound {float(bound[r, c])}")


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dot64(a, w):
    """(a @ W^T, |a| @ |W|^T) in float64; a [..., M, K], w [N, K], both taken as data."""
    a64, w64 = a.double(), w.double()
    return a64 @ w64.t(), a64.abs() @ w64.abs().t()


def _zeros_like_cols(t):
    return torch.zeros(t.shape[-1], dtype=torch.float64, device=t.device)


def pre_bound(dot, mag, K, bias=None):
    """(pre, e_pre): the biased product in float64 and the bound of the kernel's f32 value of it."""
    b = bias.double() if bias is not None else _zeros_like_cols(dot)
    pre = dot + b
    return pre, C_DOT * K * U * mag + U * pre.abs() + 2 * U * b.abs()


def gemm_ref_bound(dot, mag, K, *, bias=None, residual=None, gelu=False):
    """(ref, bound) of C = [gelu](a @ W^T + bias) [+ residual] as an f32 value; residual broadcastable to dot."""
    b = bias.double() if bias is not None else _zeros_like_cols(dot)
    pre = dot + b
    r = residual.double() if residual is not None else None
    if gelu:
        _, e_pre = pre_bound(dot, mag, K, bias)
        ref = gelu64(pre)
        if r is not None:
            ref = ref + r
        e = GELU_SLOPE * e_pre + GELU_ABS + U * ref.abs()
        if r is not None:
            e = e + 2 * U * r.abs()
        return ref, e
    ref = pre + r if r is not None else pre
    e = C_DOT * K * U * mag + U * ref.abs() + 2 * U * (b.abs() + (r.abs() if r is not None else 0.0))
    return ref, e


def swiglu_split(t):
    """Columns of a gate / up interleaved [.., N] tensor (blocks of 16 gate columns, then their 16 up columns) -> (gate, up),
    each [.., N / 2]."""
    v = t.reshape(*t.shape[:-1], t.shape[-1] // 32, 2, 16)
    return v[..., 0, :].reshape(*t.shape[:-1], -1), v[..., 1, :].reshape(*t.shape[:-1], -1)


def swiglu_ref_bound(dot, mag, K, *, bias=None):
    """(ref, bound) of silu(gate) * up over interleaved columns: the formula of test_gpu_decode_plan.py with the bias terms of
    the f32 bound in e_g / e_u."""
    pre, e = pre_bound(dot, mag, K, bias)
    gate, up = swiglu_split(pre)
    eg, eu = swiglu_split(e)
    sg = gate * torch.sigmoid(gate)
    ref = sg * up
    return ref, SILU_SLOPE * eg * (up.abs() + eu) + sg.abs() * eu + U * (16 + 4 * gate.abs()) * ref.abs()


def bf16_out_bound(bound, ref, out):
    return bound + bf16_ulp(torch.maximum(ref.abs(), out.double().abs()))


def within(got, ref, bound):
    """Mask of the elements inside the bound (NaN counts as outside)."""
    return (got.double() - ref).abs() <= bound


def worst_ratio(got, ref, bound):
    """max err / bound over the elements (bound 0 with err 0 counts as 0)."""
    err = (got.double() - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


# ---- norms --------------------------------------------------------------------------------------------------------------------
def norm_depth(N):
    """Summation depth of the norm kernels' reductions: a lane's serial chain of N / 256 vectors of 4, the 6-level shuffle
    tree, 2 for a partly filled last chunk."""
    return N / 64.0 + 8.0


def norm_ref_bound(x, gamma, beta, eps, *, rms=False, res=None, alpha=1.0):
    """(ref, bound) of y = (z - mean) rstd gamma + beta (LayerNorm) or z rstd gamma (RMSNorm), z = x + alpha res, as an f32
    value, per element in float64.  x [M, N] is taken as data.  Derivation: test_gpu_norm_exact.py."""
    N = x.shape[-1]
    D = norm_depth(N)
    g = gamma.double()
    z = x.double()
    dz = torch.zeros_like(z)
    if res is not None:
        ar = alpha * res.double()
        z = z + ar
        dz = U * (ar.abs() + z.abs())                      # round(alpha r), round(x + .)
    if rms:
        s = z.pow(2).mean(-1, keepdim=True)
        t = s + eps
        dt = (2 * z.abs() * dz + dz * dz).mean(-1, keepdim=True) + (D + 3) * U * t
        rstd = torch.rsqrt(t)
        rho = 0.5 * dt / t + 2 * U                         # d rstd / rstd; 2u = one ulp of rsqrtf
        ref = z * rstd * g
        return ref, g.abs() * rstd * (dz + (z.abs() + dz) * (rho + 2 * U))
    b = beta.double()
    mean = z.mean(-1, keepdim=True)
    e_m = D * U * z.abs().mean(-1, keepdim=True) + U * mean.abs() + dz.mean(-1, keepdim=True)
    d = z - mean
    e_d = e_m + dz + U * d.abs()
    t = d.pow(2).mean(-1, keepdim=True) + eps
    dt = (2 * d.abs() * e_d + e_d * e_d).mean(-1, keepdim=True) + (D + 3) * U * t
    rstd = torch.rsqrt(t)
    rho = 0.5 * dt / t + 2 * U
    ref = d * rstd * g + b
    return ref, g.abs() * rstd * (e_d + (d.abs() + e_d) * (rho + 3 * U)) + U * ref.abs()


# ---- glue and audio front-end kernels (tests/test_glue_bounds.py on the CPU, test_gpu_glue_exact.py / test_gpu_frontend_exact.py) --
F64_SLACK = 2.0 ** -30     # the float64 slack of the front-end bounds: test_glue_bounds.py measures two independent float64
#                            formulations (rfft; a direct DFT summed in reverse order) and asserts they differ by < F64_SLACK / 8


def bf16_rne(x):
    """float64 -> the nearest bf16 value (ties to even), returned as float64.  Done on the exponent / mantissa of the double
    itself: a cast through float32 rounds twice.  Subnormals are spaced 2^-133; +-0 stay; no overflow handling (not needed)."""
    _, ex = torch.frexp(x)                                   # |x| = m 2^ex, m in [0.5, 1)
    ulp = torch.exp2((ex - 1).clamp_min(-126).double() - 7)
    return torch.round(x / ulp) * ulp                        # the division is exact; torch.round is half-to-even


def bf16_interval(ref, e):
    """(lo, hi) = (bf16(ref - e), bf16(ref + e)) under round-to-nearest-even: rounding is monotone, so a kernel whose f32 value
    is within e of ref and which rounds it once to bf16 lands in [lo, hi]; one that truncates, or rounds an ulp too far, does
    not hide inside an added output ulp."""
    return bf16_rne(ref - e), bf16_rne(ref + e)


def in_interval(out, lo, hi):
    """Mask of the bf16 outputs inside [lo, hi] (NaN counts as outside)."""
    o = out.double()
    return (lo <= o) & (o <= hi)


def interval_ratio(out, ref, lo, hi):
    """The err / bound figure of an interval check: max of |out - ref| / (the interval's reach on that side); > 1 iff outside."""
    o = out.double()
    err = (o - ref).abs()
    reach = torch.where(o > ref, hi - ref, ref - lo)
    r = torch.where(err == 0, torch.zeros_like(err), err / reach)
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def rope_ref_bound(x, cos, sin):
    """(ref, e) of the HF rotate-half RoPE of x [..., D] (bf16, taken as data) by cos / sin [..., D / 2] (f32, as data,
    broadcastable): with a = x[..., :D/2], b = x[..., D/2:],  ref_lo = a c - b s,  ref_hi = b c + a s.
    rope_rot8 (csrc/common.h) rounds each product and the sum once (__fmul_rn / __fsub_rn, no contraction):
        e = U (|a c| + |b s|) + U |ref|        (the two products; the sum, whose ulp is that of ref to first order)."""
    h = x.shape[-1] // 2
    a, b = x[..., :h].double(), x[..., h:].double()
    c, s = cos.double(), sin.double()
    lo, hi = a * c - b * s, b * c + a * s
    e_lo = U * ((a * c).abs() + (b * s).abs()) + U * lo.abs()
    e_hi = U * ((b * c).abs() + (a * s).abs()) + U * hi.abs()
    return torch.cat([lo, hi], -1), torch.cat([e_lo, e_hi], -1)


def f32_scalar(v):
    """The value a float argument has once the C ABI has made it an f32."""
    return float(torch.tensor(v, dtype=torch.float32))


def axpby_ref_bound(x, alpha, add=None):
    """(ref, e) of x alpha (+ add) as an f32 value; alpha is what the kernel receives (f32).  Unfused, fl(fl(x alpha) + add)
    is off by at most U |x alpha| + U |ref|; the fused form by U |ref| alone: e = U |x alpha| + U |ref| admits both.  Without
    `add` there is one rounding: e = U |ref|."""
    p = x.double() * f32_scalar(alpha)
    if add is None:
        return p, U * p.abs()
    ref = p + add.double()
    return ref, U * p.abs() + U * ref.abs()


def lora_ref_bound(x, a, scale):
    """(ref, e) of scale * x @ a^T, x [M, K0] and a [r, K0] bf16 taken as data.  A lane of lora_down_kernel sums K0 / 64
    exact bf16 products in series (K0 / 512 steps of 8), the wave adds 6 shuffle levels, 2 spare for the ragged last step:
        e = (K0 / 64 + 8) U |scale| sum |x a| + 2U |ref|       (2U: the product with scale, and margin for its f32 value)."""
    K0 = x.shape[-1]
    s = f32_scalar(scale)
    dot, mag = dot64(x, a)
    ref = s * dot
    return ref, (K0 / 64.0 + 8.0) * U * abs(s) * mag + 2 * U * ref.abs()


def _sigmoid_bound(s, e_s):
    """sigma = 1 / (1 + __expf(-s)) of an f32 s within e_s of the float64 s.  sigma' = sigma (1 - sigma) <= 1/4 falls with |t|,
    so over [s - e_s, s + e_s] it is at most its value at the point nearest 0, t = max(|s| - e_s, 0) (the mean value theorem;
    tighter than the flat 1/4, which leaves a saturated sigmoid a bound thousands of times its error); __expf is exp2 of the
    rounded product s log2(e), within (|s| + 3) U relative, which moves sigma by sigma (1 - sigma) times that; the sum 1 + e
    and the division are two roundings, 2 more on the same factor and 2U sigma:
        e_sigma = e_s sigma'(t) + (|s| + 5) U sigma (1 - sigma) + 2U sigma."""
    sg = torch.sigmoid(s)
    t = (s.abs() - e_s).clamp_min(0.0)
    return sg, e_s * torch.sigmoid(t) * torch.sigmoid(-t) + (s.abs() + 5) * U * sg * torch.sigmoid(-s) + 2 * U * sg


def gate_ref_bound(q, w, b, a):
    """(ref, e) of the BEATs gate  sigma(s_a) (sigma(s_b) A_h - 1) + 2,  q [M, H, 64] bf16 as data, w [8, 64], b [8], a [H] f32:
    s_a / s_b are the sums of the accumulators 0..3 / 4..7, each b_j + 64 serial products (65 terms) and 3 more additions:
        e_s = 70 U sum_j (sum_d |w_jd q_d| + |b_j|),
        e   = e_sa |sigma_b A - 1| + sigma_a |A| e_sb + 4U (|ref| + 2)
    (the last: the product with A, the - 1, the outer product and the + 2, on values no larger than |ref| + 2)."""
    q64, w64, b64 = q.double(), w.double(), b.double()
    proj = q64 @ w64.t() + b64                                 # [M, H, 8]
    mag = q64.abs() @ w64.abs().t() + b64.abs()
    s = proj.view(*proj.shape[:-1], 2, 4).sum(-1)
    e_s = 70 * U * mag.view(*mag.shape[:-1], 2, 4).sum(-1)
    sa, e_a = _sigmoid_bound(s[..., 0], e_s[..., 0])
    sb, e_b = _sigmoid_bound(s[..., 1], e_s[..., 1])
    A = a.double()
    ref = sa * (sb * A - 1.0) + 2.0
    return ref, e_a * (sb * A - 1.0).abs() + sa * A.abs() * e_b + 4 * U * (ref.abs() + 2)


def ce_ref_bound(logits, labels):
    """(row_ref, row_e, mean_ref, mean_e) of the ignore_index cross entropy; logits [M, V] f32 as data, labels [M] (a label
    outside [0, V) is ignored: its row is 0 exactly, bound 0).  m = max x, d = x - m, p = softmax, l = log sum e^d,
    ref = l + m - x_y.  ce_rows_kernel: d is rounded once (U |d|), __expf of it is within (|d| + 3) U relative, so each term
    of the sum carries (2 |d| + 3) U relative and the sum moves by U sum p (2 |d| + 3) relative — absolute in l, its log; a
    thread's chain of V / 256 additions, the shuffle tree and the four wave sums of positive terms add (V / 256 + 8) U; logf
    2U |l|; the two additions U |l + m| and U |ref|; terms flushed below the smallest normal, 1e-37 V:
        e = (V / 256 + 8) U + U sum_v p_v (2 |d_v| + 3) + 2U |l| + U |l + m| + U |ref| + 1e-37 V.
    The mean over the n valid rows is a sum of M / 256 serial terms per thread, the tree, and one division:
        e_mean = (M / 256 + 8) U mean |ref_row| + mean e_row + U |mean|;  no valid row: NaN (mean_e 0)."""
    M, V = logits.shape
    x = logits.double()
    y = labels.long()
    valid = (y >= 0) & (y < V)
    m = x.max(-1, keepdim=True).values
    d = x - m
    ex = torch.exp(d)
    z = ex.sum(-1, keepdim=True)
    p = ex / z
    l = torch.log(z)
    xy = x.gather(1, y.clamp(0, V - 1)[:, None])
    ref = l + m - xy
    e = ((V / 256.0 + 8.0) * U + U * (p * (2 * d.abs() + 3)).sum(-1, keepdim=True) + 2 * U * l.abs() + U * (l + m).abs()
         + U * ref.abs() + 1e-37 * V)
    ref = torch.where(valid, ref[:, 0], torch.zeros_like(ref[:, 0]))
    e = torch.where(valid, e[:, 0], torch.zeros_like(e[:, 0]))
    n = int(valid.sum())
    if n == 0:
        return ref, e, float("nan"), 0.0
    mean = float(ref.sum() / n)
    e_mean = (M / 256.0 + 8.0) * U * float(ref.abs().sum() / n) + float(e.sum() / n) + U * abs(mean)
    return ref, e, mean, e_mean


def whisper_ref_bound(r):
    """(r, e) for one clip's float64 log-mel r = (max(l, l_max - 8) + 4) / 4 (oracle: whisper_logmel(as_f64=True)),
    l = log10(max(mel, 1e-10)).  The kernel's mel energies are float64; it rounds l to f32 (U |l|), takes the maximum of
    those (U |l_max|), subtracts 8 (U |l_max - 8|), adds 4 (U |l_c + 4|, at most U (|l_c| + 4)) and divides by 4 (exact), l_c
    the clamped value:
        e = U (2 max(|l_c|, |l_max| + 8) + 4) / 4 + U |r| + 2^-30.
    |l| is taken at the clamped value l_c = 4 r - 4 (tighter than the unclamped l, and all r gives): the rounding of an l
    below the clamp reaches the output only if it crosses the clamp, and then l is within that rounding of l_c."""
    lc = 4.0 * r - 4.0
    lmax = lc.max().abs()
    return r, U * (2 * torch.maximum(lc.abs(), lmax + 8.0) + 4.0) / 4.0 + U * r.abs() + F64_SLACK


def kaldi_ref_bound(r):
    """(r, e) for the float64 normalised fbank r (oracle: kaldi_fbank(as_f64=True) with the f32 values of mean and std, which
    is what the kernel receives): the kernel works in float64 and rounds once, e = U |r| + 2^-30."""
    return r, U * r.abs() + F64_SLACK


# ---- the sampled and the beam-search decode tails (test_decode_tail_bounds.py on the CPU, test_gpu_decode_tail_exact.py) -------
# The references and the derivations of their bounds are project code: oracle/decode_tail.py.  What follows judges one row of
# outputs — the kernel's, or those of the f32 emulation of tests/decode_tail_cases.py — against them; both checkers return
# (worst err / bound, ambiguous) and raise AssertionError.
def _ratio(err, bound):
    import numpy as np
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.nan_to_num(r, nan=float("inf")).max()) if r.size else 0.0


def _same_bits(a, b):
    import numpy as np
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32),
                          np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def check_sampler_row(case, b, out, tag=""):
    """One row of a sampler launch.  `case`: a dict of tests/decode_tail_cases.py; `out`: work [ldw], ids / probs [cap],
    count, next_id, tokens [width], finished.  Always: the scores bit for bit (NaN where NaN), every sentinel, the kept ids
    (exact: their order does not depend on any sum), count in [keep_lo, keep_hi], each probability within its bound of the
    float64 value renormalised over the kernel's own count, a justified pick, the bookkeeping.  On a determinate row also
    count == keep and the float64 pick."""
    import numpy as np
    from oracle import decode_tail as dt
    V, step, S = case["V"], case["step"], case["sentinel"]
    row = case["logits"][b, :V]
    prev = case["tokens"][b, :step]
    scores = dt.sampler_scores(row, prev, case["pen"], case["temp"])
    work = np.asarray(out["work"], dtype=np.float32)
    nan = np.isnan(scores)
    assert np.array_equal(np.isnan(work[:V]), nan), f"{tag}: NaN pattern of the scores"
    assert _same_bits(np.where(nan, 0, work[:V]), np.where(nan, 0, scores)), \
        f"{tag}: scores differ from the two f32 operations at {np.nonzero(np.where(nan, 0, work[:V]) != np.where(nan, 0, scores))[0][:5]}"
    assert _same_bits(work[V:], np.full(work.shape[0] - V, S, np.float32)), f"{tag}: work written past V"
    ref = dt.SamplerRef(scores, case["top_k"], case["top_p"])
    cnt = int(out["count"])
    assert ref.keep_lo <= cnt <= ref.keep_hi, f"{tag}: count {cnt} outside [{ref.keep_lo}, {ref.keep_hi}]"
    ids = np.asarray(out["ids"])
    assert ids[:cnt].tolist() == ref.cand[:cnt].tolist(), f"{tag}: kept ids"
    assert bool((ids[cnt:] == -1).all()), f"{tag}: debug ids written past count"
    probs = np.asarray(out["probs"], dtype=np.float32)
    assert _same_bits(probs[cnt:], np.full(probs.shape[0] - cnt, S, np.float32)), f"{tag}: debug probs written past count"
    cdf, e_cdf, p64, e_p = ref.kept(cnt)
    assert bool(np.isfinite(probs[:cnt]).all()), f"{tag}: non-finite probability"
    err = np.abs(probs[:cnt].astype(np.float64) - p64)
    ratio = _ratio(err, e_p)
    assert bool((err <= e_p).all()), f"{tag}: probability outside its bound, worst err/bound {ratio}"
    fin_in, nxt = int(case["finished"][b]), int(out["next_id"])
    u = case["u"][b]
    if fin_in:
        assert nxt == case["pad"], f"{tag}: finished row emitted {nxt}"
    else:
        ok = ref.cand[ref.justified_picks(u, cnt)].tolist()
        assert nxt in ok, f"{tag}: pick {nxt} not justified by u={u!r} (justified: {ok})"
    j64, pick_det = ref.pick(u, ref.keep)
    determinate = ref.cut_determinate and pick_det
    if determinate:
        assert cnt == ref.keep, f"{tag}: determinate row, count {cnt} != {ref.keep}"
        if not fin_in:
            assert nxt == int(ref.cand[j64]), f"{tag}: determinate row, pick {nxt} != {int(ref.cand[j64])}"
    want_fin = int(bool(fin_in) or nxt in [e for e in case["eos"] if e >= 0])
    assert int(out["finished"]) == want_fin, f"{tag}: finished flag"
    toks = np.asarray(out["tokens"])
    want = case["tokens"][b].copy()
    want[step] = nxt
    assert toks.tolist() == want.tolist(), f"{tag}: out_tokens"
    return ratio, not determinate


def check_beam_row(ref, out, old, tag=""):
    """One batch row of a beam-step launch against `ref` (oracle.decode_tail.BeamStepRef, built from the incoming state
    `old`).  `out` / `old`: dicts of the row's run_score [K], run_seq [K, T], fin_score, fin_seq, fin_len, fin_flag, unsat
    and (out) next_ids, parent (beam index inside the row).  Always: ranges; each running sequence is its parent's old one
    with the token at `step`; run_score within the bound of the float64 score of the (parent, token) chosen, and that score
    within the bounds of the reference's i-th best run value (the rank it took); a closed row keeps its finished slots bit
    for bit.  On a determinate step every integer equals the reference and fin_score is within its bound."""
    import numpy as np
    K, V, T, step = ref.K, ref.V, ref.T, ref.step
    par, nxt = np.asarray(out["parent"]).astype(np.int64), np.asarray(out["next_ids"]).astype(np.int64)
    assert bool(((par >= 0) & (par < K)).all()) and bool(((nxt >= 0) & (nxt < V)).all()), f"{tag}: parent / token range"
    want_seq = np.asarray(old["run_seq"])[par].copy()
    want_seq[np.arange(K), step] = nxt
    assert np.array_equal(np.asarray(out["run_seq"]), want_seq), f"{tag}: run_seq is not parent's sequence + token"
    assert int(out["unsat"]) in (0, 1) and set(np.asarray(out["fin_flag"]).tolist()) <= {0, 1}, f"{tag}: flags"
    assert bool(((np.asarray(out["fin_len"]) >= 0) & (np.asarray(out["fin_len"]) <= T)).all()), f"{tag}: fin_len range"
    errs, bounds = [], []
    rs = np.asarray(out["run_score"], dtype=np.float64)
    for i in range(K):
        a, e = ref.score_of(int(par[i]), int(nxt[i]))
        if np.isfinite(a):
            errs.append(abs(rs[i] - a)); bounds.append(e)
            assert abs(rs[i] - a) <= e, f"{tag}: run_score[{i}] {rs[i]} vs {a}, bound {e}"
            assert abs(a - ref.run_score[i]) <= e + ref.run_score_e[i], f"{tag}: beam {i} took a rank its score does not justify"
        else:
            assert rs[i] == a and ref.run_score[i] == a, f"{tag}: run_score[{i}] {rs[i]} vs {a}"
    if not ref.row_open:
        for name in ("fin_seq", "fin_len", "fin_flag"):
            assert np.array_equal(np.asarray(out[name]), np.asarray(old[name])), f"{tag}: closed row, {name} changed"
        assert _same_bits(out["fin_score"], old["fin_score"]) and int(out["unsat"]) == 0, f"{tag}: closed row changed"
    if ref.determinate:
        assert par.tolist() == ref.parent.tolist() and nxt.tolist() == ref.next_ids.tolist(), \
            f"{tag}: parents / tokens {par.tolist()} {nxt.tolist()} vs {ref.parent.tolist()} {ref.next_ids.tolist()}"
        assert np.array_equal(np.asarray(out["fin_flag"]), ref.fin_flag), f"{tag}: fin_flag"
        assert np.array_equal(np.asarray(out["fin_len"]), ref.fin_len), f"{tag}: fin_len"
        assert np.array_equal(np.asarray(out["fin_seq"]), ref.fin_seq), f"{tag}: fin_seq"
        assert int(out["unsat"]) == ref.unsat, f"{tag}: unsat {int(out['unsat'])} vs {ref.unsat}"
        fs = np.asarray(out["fin_score"], dtype=np.float64)
        for i in range(K):
            errs.append(abs(fs[i] - ref.fin_score[i])); bounds.append(ref.fin_score_e[i])
            assert abs(fs[i] - ref.fin_score[i]) <= ref.fin_score_e[i], \
                f"{tag}: fin_score[{i}] {fs[i]} vs {ref.fin_score[i]}, bound {ref.fin_score_e[i]}"
    return _ratio(errs, bounds), not ref.determinate

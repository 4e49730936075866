"""icl_layernorm / icl_rmsnorm: every output element against float64, with a bound derived from the kernels' structure (`-m gpu`).

Outputs start as NaN inside a sentinel allocation (a guard row above and below, 8 pad columns); inputs are views with
ldx = N + 8 whose pad columns hold NaN (NaN * 0 is NaN: a read past N poisons the row).

The bound (tests/fp64_bounds.py: norm_ref_bound; first order in u = 2^-24, the squares of the input errors kept)
  Structure (csrc/norm.hip): a row is owned by one 64-lane wave and stays in registers.  A lane adds its at most N / 256 vectors
  of 4 elements in a serial chain, then the wave runs a 6-level shuffle tree; the streaming kernel's lanes own 8-element chunks
  instead, the same N / 64 elements per lane.  An element therefore passes through at most D = N / 64 + 8 roundings of a sum
  (chain + tree + 2 for a partly filled last chunk), not N, and a sum of terms t_i carries at most D u sum |t_i|.  (D is
  charged to every element; the exact worst chain exceeds it by one rounding, for the elements of the lanes that own a partly
  filled last chunk only — N = 772: 21 against 20.1, N = 1280 on the streaming kernel: 29 against 28 — which the elements of
  the other lanes, charged D too, more than pay for unless the row's mass sits in those lanes alone.)
  Input  z_i = x_i + alpha r_i (no residual: z = x exactly): dz_i = u (|alpha r_i| + |z_i|)  (round(alpha r), round(x + .)).
  Mean   m^ = fl(sum z^) / N:    e_m = D u mean|z| + u |m| + mean(dz)          (the sum, the division, the inputs)
  d_i    d^_i = fl(z^_i - m^):   e_d,i = e_m + dz_i + u |d_i|
  t      t = mean(d^2) + eps:    dt = mean(2 |d_i| e_d,i + e_d,i^2) + (D + 3) u t
                                 (each square: the error of d^ and one rounding; the sum: D; the division and the + eps: 2)
  rstd   rsqrtf(t^):             rho = dt / (2 t) + 2u relative               (2u = one ulp of rsqrtf)
  y_i    ((d^_i rstd^) g_i) + b_i: |y^_i - y_i| <= |g_i| rstd (e_d,i + (|d_i| + e_d,i) (rho + 3u)) + u |y_i|
                                 (two products and the sum, or a product and an fma)
  RMSNorm: no mean, d = z, t = mean(z^2) + eps with dt = mean(2 |z_i| dz_i + dz_i^2) + (D + 3) u t, y_i = (z_i rstd^) g_i:
           |y^_i - y_i| <= |g_i| rstd (dz_i + (|z_i| + dz_i) (rho + 2u)).
  bf16 outputs: + 1 bf16 ulp of max(|ref|, |out|).  out2 (always bf16) == bf16(out) exactly when out is f32.
The two-pass statistics are what keeps e_d at D u mean|z|: on a row with mean 1000 and std 1 a one-pass E[x^2] - mean^2 loses
the variance in f32 and leaves this bound by orders of magnitude (tests/test_fp64_bounds.py shows that on the CPU)."""
import pytest
import torch

import fp64_bounds as fb
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENT = 7.0
EPS = 1e-5
WORST = {"norms": 0.0, "where": ""}
NS = (768, 772, 1280, 1284, 1536, 4096, 5120, 5124, 8192)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print(f"\nworst err/bound, norms: {WORST['norms']:.4f} ({WORST['where']})")


def _randn(shape, seed, dtype=torch.float32):
    g = torch.Generator(DEV).manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV).to(dtype)


def _padded_input(data, dtype):
    """data [M, N] as a view of a [M, N + 8] tensor whose pad columns hold NaN."""
    M, N = data.shape
    store = torch.full((M, N + 8), float("nan"), dtype=dtype, device=DEV)
    store[:, :N] = data
    return store[:, :N]


def _guarded(M, N, dtype, pad=8):
    buf = torch.full((M + 2, N + pad), SENT, dtype=dtype, device=DEV)
    view = buf[1:M + 1, :N]
    view.fill_(float("nan"))
    return buf, view


def _assert_guard(buf, view, what):
    chk = buf.clone()
    chk[1:1 + view.shape[0], :view.shape[1]] = SENT
    assert bool((chk == SENT).all()), f"{what}: wrote outside its M x N output"


def _params(N, seed=0):
    return 1 + 0.5 * _randn((N,), 70 + seed), _randn((N,), 71 + seed)


def _check(out, x, g, b, what, rms=False, res=None, alpha=1.0, chunk=4096):
    for r0 in range(0, x.shape[0], chunk):
        sl = slice(r0, r0 + chunk)
        ref, e = fb.norm_ref_bound(x[sl], g, b, EPS, rms=rms, res=None if res is None else res[sl], alpha=alpha)
        if out.dtype == torch.bfloat16:
            e = fb.bf16_out_bound(e, ref, out[sl])
        fb.assert_within(out[sl], ref, e, f"{what}, rows from {r0}")
        ratio = fb.worst_ratio(out[sl], ref, e)
        if ratio > WORST["norms"]:
            WORST["norms"], WORST["where"] = ratio, what


def _launch(B, rms, x, g, b, out, **kw):
    if rms:
        B.rmsnorm(x, g, out, EPS, **kw)
    else:
        B.layernorm(x, g, b, out, EPS, **kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("in_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
def test_norm_every_element(B, N, in_dtype, rms):
    """37 rows (ten blocks of 4 rows, the last one ragged) at every instantiation and chunk fill: 768 / 772 (MAXV 3 / 5, a
    partly filled last chunk), 1280 / 1284, 1536 (the streaming kernel, 3 chunks), 4096, 5120 (streaming, 10 chunks) / 5124,
    8192 (MAXV 32); N % 8 != 0 forces the row kernel.  Both output types; LayerNorm into f32 also writes out2."""
    M = 37
    x = _padded_input(_randn((M, N), 80 + N) * 2 + 0.5, in_dtype)
    g, b = _params(N)
    for od in (torch.float32, torch.bfloat16):
        buf, out = _guarded(M, N, od)
        what = f"{'rms' if rms else 'ln'} N={N} {in_dtype} -> {od}"
        if not rms and od == torch.float32:
            buf2, out2 = _guarded(M, N, torch.bfloat16)
            _launch(B, rms, x, g, b, out, out2=out2)
            assert torch.equal(out2.view(torch.int16), out.to(torch.bfloat16).view(torch.int16)), f"{what}: out2 != bf16(out)"
            _assert_guard(buf2, out2, what + " out2")
            _check(out, x, g, b, what + " +out2", rms)
            _assert_guard(buf, out, what)
            buf, out = _guarded(M, N, od)
        _launch(B, rms, x, g, b, out)
        _check(out, x, g, b, what, rms)
        _assert_guard(buf, out, what)


@pytest.mark.parametrize("N", [768, 772, 1536])
def test_layernorm_beats_form(B, N):
    """BEATs' deep-norm step, layernorm(o, g, b, x, res=x, alpha, out2=xb): y = LN(o + alpha x) written over x (the output
    aliases the residual), and its bf16 copy.  The reference is taken from clones of the inputs."""
    M, alpha = 70, 1.7
    xbuf, x = _guarded(M, N, torch.float32)
    x.copy_(_randn((M, N), 90 + N))
    o = _padded_input(_randn((M, N), 91 + N) * 2 + 0.5, torch.float32)
    x0, o0 = x.clone(), o.clone()
    g, b = _params(N, 1)
    buf2, xb = _guarded(M, N, torch.bfloat16)
    B.layernorm(o, g, b, x, EPS, res=x, alpha=alpha, out2=xb)
    torch.cuda.synchronize()
    assert torch.equal(o, o0)
    _check(x, o0, g, b, f"BEATs form N={N}", res=x0, alpha=alpha)
    assert torch.equal(xb.view(torch.int16), x.to(torch.bfloat16).view(torch.int16))
    _assert_guard(xbuf, x, "BEATs form out")
    _assert_guard(buf2, xb, "BEATs form out2")


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
def test_norm_misaligned_bf16_input(B, rms):
    """A bf16 x that is 8-byte but not 16-byte aligned at N = 1536: the streaming kernel's 16-B loads are out, the launch must
    take the row kernel (8-B loads) and stay inside the bound."""
    M, N = 37, 1536
    flat = torch.full((M * N + 8,), float("nan"), dtype=torch.bfloat16, device=DEV)
    data = (_randn((M, N), 95) * 2 + 0.5).to(torch.bfloat16)
    flat[4:4 + M * N] = data.reshape(-1)
    x = flat[4:4 + M * N].view(M, N)
    assert x.data_ptr() % 16 == 8
    g, b = _params(N, 2)
    for od in (torch.float32, torch.bfloat16):
        buf, out = _guarded(M, N, od)
        _launch(B, rms, x, g, b, out)
        _check(out, x, g, b, f"misaligned x -> {od}", rms)
        _assert_guard(buf, out, "misaligned x")


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
def test_norm_hoist_switch(B, rms):
    """norm_kernel loads gamma / beta ahead of the reductions (HOIST) up to M = 2048 rows and inside the store loop above: same
    values, same arithmetic.  N = 1280 on the row kernel (LayerNorm: the dual-output form; RMSNorm: ldy = N + 4, not a
    multiple of 8) at M = 2048 and 2049: every row inside the bound, row 100 — every shared row — bit-identical."""
    N = 1280
    x = _randn((2049, N), 96) * 2 + 0.5
    g, b = _params(N, 3)
    outs = []
    for M in (2048, 2049):
        buf, out = _guarded(M, N, torch.float32, pad=4 if rms else 8)
        if rms:
            _launch(B, True, x[:M], g, b, out)
        else:
            buf2, out2 = _guarded(M, N, torch.bfloat16)
            _launch(B, False, x[:M], g, b, out, out2=out2)
            assert torch.equal(out2.view(torch.int16), out.to(torch.bfloat16).view(torch.int16))
            _assert_guard(buf2, out2, "HOIST out2")
        _check(out, x[:M], g, b, f"HOIST switch M={M}", rms)
        _assert_guard(buf, out, f"HOIST switch M={M}")
        outs.append(out)
    assert torch.equal(outs[0][100].view(torch.int32), outs[1][100].view(torch.int32))
    assert torch.equal(outs[0].contiguous().view(torch.int32), outs[1][:2048].contiguous().view(torch.int32))


@pytest.mark.parametrize("rms,in_dtype,out_dtype", [(False, torch.float32, torch.bfloat16), (True, torch.bfloat16, torch.float32)],
                         ids=["ln-f32-bf16", "rms-bf16-f32"])
def test_norm_streaming_persistent_loop(B, rms, in_dtype, out_dtype):
    """The streaming kernel at N = 1536 with M = 4 * n_waves + 3 rows: launch_norm's grid is min((M + 3) / 4, 8 n_cu) blocks of
    4 waves, so every wave walks four rows (prefetching the next under the current one) and the first three a fifth.  Every row
    against float64; the first, a middle and the last row of each pass also bit for bit against a launch of those rows alone."""
    N = 1536
    n_waves = 4 * 8 * B.device_cu_count()
    M = 4 * n_waves + 3
    assert (M + 3) // 4 > n_waves // 4
    x = (_randn((M, N), 97) * 2 + 0.5).to(in_dtype)
    g, b = _params(N, 4)
    buf, out = _guarded(M, N, out_dtype)
    _launch(B, rms, x, g, b, out)
    _check(out, x, g, b, f"persistent loop M={M}", rms)
    _assert_guard(buf, out, "persistent loop")
    rows = [p * n_waves + r for p in range(4) for r in (0, n_waves // 2 + p, n_waves - 1)] + [4 * n_waves, M - 1]
    idx = torch.tensor(rows, device=DEV)
    few = torch.full((len(rows), N), float("nan"), dtype=out_dtype, device=DEV)
    _launch(B, rms, x[idx].contiguous(), g, b, few)
    assert torch.equal(few.view(torch.int16), out[idx].contiguous().view(torch.int16))


@pytest.mark.parametrize("N", [768, 1536, 8192])
def test_norm_hard_rows(B, N):
    """An all-zero row (LayerNorm gives beta exactly, RMSNorm 0: rstd = eps^-1/2 is finite), a constant row (the variance is
    the rounding noise of the mean, amplified by eps^-1/2: the bound carries e_m * rstd) and a row with mean 1000 and std 1,
    where only two-pass statistics keep the variance."""
    M = 8
    data = _randn((M, N), 98 + N) * 2 + 0.5
    data[2] = 0.0
    data[4] = 3.0
    data[6] = 1000.0 + _randn((N,), 99)
    x = _padded_input(data, torch.float32)
    g, b = _params(N, 5)
    for rms in (False, True):
        for od in (torch.float32, torch.bfloat16):
            buf, out = _guarded(M, N, od)
            _launch(B, rms, x, g, b, out)
            assert bool(torch.isfinite(out).all())
            want0 = torch.zeros(N, device=DEV) if rms else b
            assert torch.equal(out[2], want0.to(od)), "the all-zero row"
            _check(out, x, g, b, f"hard rows N={N} rms={rms} -> {od}", rms)
            _assert_guard(buf, out, "hard rows")

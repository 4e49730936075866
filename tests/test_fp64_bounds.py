"""The per-element float64 bounds of tests/fp64_bounds.py, checked on the CPU without the kernels: each bound lets a correct
f32 implementation through at every element, and each bites — a float64 reference with one deliberate mistake leaves it at the
mistaken elements and nowhere else.

Case: M = 8, N = 64, K = 256 (norms: 8 rows of 64, row 5 with mean 1000 and std 1); inputs as in the GPU tests (activations
randn * 0.5, weights randn * 0.075, bias and residual O(1)).  "Correct" is plain PyTorch on the CPU: bf16 inputs, f32
accumulation and epilogue, a bf16 rounding where the kernel rounds its output."""
import pytest
import torch

import fp64_bounds as fb

M, N, K = 8, 64, 256
EPS = 1e-5


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def case():
    a = (_randn(M, K, seed=1) * 0.5).to(torch.bfloat16)
    w = (_randn(N, K, seed=2) * 0.075).to(torch.bfloat16)
    bias = _randn(N, seed=3)
    res = _randn(M + 1, N, seed=4)                    # one spare row for the "residual of row m + 1" mutant
    dot, mag = fb.dot64(a, w)
    return dict(a=a, w=w, bias=bias, res=res, dot=dot, mag=mag, acc=a.float() @ w.float().t())


def _outside(got, ref, bound):
    return ~fb.within(got, ref, bound)


def _only(mask, rows, cols):
    want = torch.zeros_like(mask)
    want[rows, cols] = True
    return torch.equal(mask, want), f"outside at {mask.nonzero().tolist()}, expected rows {rows} cols {cols}"


# ---- a correct result stays inside ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("epi", ["plain", "bias", "bias_res", "bias_res_bf16", "gelu", "bias_gelu", "bias_gelu_res"])
def test_f32_torch_gemm_is_inside_the_bound(case, epi, out_dtype):
    c = case
    bias = c["bias"] if "bias" in epi else None
    res = c["res"][:M] if "res" in epi else None
    if res is not None and epi.endswith("bf16"):
        res = res.to(torch.bfloat16)
    v = c["acc"] + bias if bias is not None else c["acc"].clone()
    if "gelu" in epi:
        v = torch.nn.functional.gelu(v)
    if res is not None:
        v = v + res.float()
    got = v.to(out_dtype)
    ref, e = fb.gemm_ref_bound(c["dot"], c["mag"], K, bias=bias, residual=res, gelu="gelu" in epi)
    if out_dtype == torch.bfloat16:
        e = fb.bf16_out_bound(e, ref, got)
    assert int(_outside(got, ref, e).sum()) == 0, fb.worst_ratio(got, ref, e)
    assert fb.worst_ratio(got, ref, e) > 1e-4          # and the bound is not absurdly wide for it


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_bias", [False, True])
def test_f32_torch_swiglu_is_inside_the_bound(case, with_bias, out_dtype):
    c = case
    bias = c["bias"] if with_bias else None
    v = c["acc"] + bias if with_bias else c["acc"]
    g, u = fb.swiglu_split(v)
    got = (torch.nn.functional.silu(g) * u).to(out_dtype)
    ref, e = fb.swiglu_ref_bound(c["dot"], c["mag"], K, bias=bias)
    if out_dtype == torch.bfloat16:
        e = fb.bf16_out_bound(e, ref, got)
    assert got.shape == (M, N // 2) and int(_outside(got, ref, e).sum()) == 0


# ---- every mutant of the reference leaves the bound where it was mutated, and only there -----------------------------------------
def test_a_dropped_k_product_is_outside(case):
    c = case
    for out_dtype in (torch.float32, torch.bfloat16):
        ref, e = fb.gemm_ref_bound(c["dot"], c["mag"], K, bias=c["bias"])
        got = ref.clone()
        got[3, 17] -= c["a"][3, 100].double() * c["w"][17, 100].double()
        if out_dtype == torch.bfloat16:
            got = got.to(torch.bfloat16)
            base = ref.to(torch.bfloat16)
            assert int(_outside(base, ref, fb.bf16_out_bound(e, ref, base)).sum()) == 0
            e = fb.bf16_out_bound(e, ref, got)
        ok, why = _only(_outside(got, ref, e), [3], [17])
        assert ok, why


def test_a_missing_bias_column_is_outside(case):
    c = case
    ref, e = fb.gemm_ref_bound(c["dot"], c["mag"], K, bias=c["bias"], residual=c["res"][:M])
    got = ref.clone()
    got[:, 41] -= c["bias"][41].double()
    ok, why = _only(_outside(got, ref, e), slice(None), [41])
    assert ok, why


def test_the_residual_of_the_next_row_is_outside(case):
    c = case
    for gelu in (False, True):
        ref, e = fb.gemm_ref_bound(c["dot"], c["mag"], K, bias=c["bias"], residual=c["res"][:M], gelu=gelu)
        got = ref.clone()
        got[2] += (c["res"][3] - c["res"][2]).double()
        ok, why = _only(_outside(got, ref, e), [2], slice(None))
        assert ok, why


def test_two_swapped_column_fragments_are_outside(case):
    c = case
    ref, e = fb.gemm_ref_bound(c["dot"], c["mag"], K, bias=c["bias"], gelu=True)
    got = ref.clone()
    got[6, 8:12], got[6, 12:16] = ref[6, 12:16], ref[6, 8:12]
    ok, why = _only(_outside(got, ref, e), [6], slice(8, 16))
    assert ok, why


def test_gelu_after_the_residual_is_outside(case):
    c = case
    res = c["res"][:M]
    ref, e = fb.gemm_ref_bound(c["dot"], c["mag"], K, bias=c["bias"], residual=res, gelu=True)
    wrong = fb.gelu64(c["dot"] + c["bias"].double() + res.double())
    got = ref.clone()
    got[4, 30] = wrong[4, 30]
    ok, why = _only(_outside(got, ref, e), [4], [30])
    assert ok, why
    assert int(_outside(wrong, ref, e).sum()) > 0.95 * ref.numel()      # and the whole wrong tensor, nearly everywhere


def test_gate_and_up_swapped_in_one_block_are_outside(case):
    c = case
    ref, e = fb.swiglu_ref_bound(c["dot"], c["mag"], K, bias=c["bias"])
    pre = c["dot"] + c["bias"].double()
    g, u = fb.swiglu_split(pre)
    wrong = u * torch.sigmoid(u) * g
    got = ref.clone()
    got[1, 16:32] = wrong[1, 16:32]                                       # interleaved columns 32..63: the second block
    ok, why = _only(_outside(got, ref, e), [1], slice(16, 32))
    assert ok, why


# ---- norms --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows():
    x = _randn(M, N, seed=11) * 2 + 0.5
    x[5] = 1000.0 + _randn(N, seed=12)                                    # where E[x^2] - mean^2 loses everything in f32
    x[6] = 0.0
    x[7] = 3.0
    return x, 1 + 0.5 * _randn(N, seed=13), _randn(N, seed=14)


def _ln_f32(x, g, b, one_pass_rows=()):
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    for r in one_pass_rows:
        var[r] = (x[r] * x[r]).mean() - mean[r] * mean[r]
    return d * torch.rsqrt(var + EPS) * g + b


@pytest.mark.parametrize("in_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_f32_torch_norms_are_inside_the_bound(rows, in_dtype, out_dtype):
    x, g, b = rows
    x = x.to(in_dtype)
    xf = x.float()
    for rms in (False, True):
        got = (xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + EPS) * g if rms else _ln_f32(xf, g, b)).to(out_dtype)
        ref, e = fb.norm_ref_bound(x, g, b, EPS, rms=rms)
        if out_dtype == torch.bfloat16:
            e = fb.bf16_out_bound(e, ref, got)
        assert int(_outside(got, ref, e).sum()) == 0, (rms, fb.worst_ratio(got, ref, e))
    # the deep-norm form: z = x + alpha * res
    res = _randn(M, N, seed=15).to(in_dtype)
    got = _ln_f32(xf + 1.7 * res.float(), g, b).to(out_dtype)
    ref, e = fb.norm_ref_bound(x, g, b, EPS, res=res, alpha=1.7)
    if out_dtype == torch.bfloat16:
        e = fb.bf16_out_bound(e, ref, got)
    assert int(_outside(got, ref, e).sum()) == 0
    assert torch.isfinite(ref).all() and torch.isfinite(e).all()


@pytest.mark.parametrize("rms", [False, True])
def test_gamma_missing_on_one_chunk_is_outside(rows, rms):
    x, g, b = rows
    ref, e = fb.norm_ref_bound(x, g, b, EPS, rms=rms)
    g1 = g.clone()
    g1[24:32] = 1.0
    wrong, _ = fb.norm_ref_bound(x, g1, b, EPS, rms=rms)
    for out_dtype in (torch.float32, torch.bfloat16):
        got = ref.clone()
        got[2, 24:32] = wrong[2, 24:32]
        got = got.to(out_dtype)
        eo = fb.bf16_out_bound(e, ref, got) if out_dtype == torch.bfloat16 else e
        ok, why = _only(_outside(got, ref, eo), [2], slice(24, 32))
        assert ok, why


def test_one_pass_variance_on_the_mean_1000_row_is_outside(rows):
    """E[x^2] - mean^2 in f32 at mean 1000, std 1: x^2 is rounded to 0.06, so the variance is off by percents and every
    element of the row but the few within 0.04 sigma of the mean leaves the bound; the other rows (two-pass) stay inside."""
    x, g, b = rows
    ref, e = fb.norm_ref_bound(x, g, b, EPS)
    got = _ln_f32(x, g, b, one_pass_rows=(5,))
    out = _outside(got, ref, e)
    assert int(out[5].sum()) >= 0.8 * N, int(out[5].sum())
    out[5] = False
    assert int(out.sum()) == 0

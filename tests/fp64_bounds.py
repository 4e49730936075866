"""Per-element error bounds against float64, shared by test_gpu_prefill_gemm.py, test_gpu_norm_exact.py and (on the CPU, without
the kernels) test_fp64_bounds.py.  Not a test module and not a conftest: plain functions over torch tensors on any device.
The constants and the comparison come from test_gpu_decode_plan.py (u = 2^-24, C_DOT = 2, _bf16_ulp, _assert_within).

GEMM  (pre = a @ W^T + bias in float64, mag = |a| @ |W|^T, K the depth; every bound is for the kernel's f32 value)
  e_pre                = C_DOT K u mag + u |pre| + 2u |bias|
  plain / residual     = C_DOT K u mag + u |ref| + 2u (|bias| + |residual|),  ref = pre (+ residual)
  GELU (+ residual)    = 1.13 e_pre + 1.5e-6 + u |ref| (+ 2u |residual|),     ref = gelu(pre) (+ residual)
                         1.13 >= sup |gelu'|; 1.5e-6 is the absolute-error contract of gelu_erf2 (csrc/common.h)
  SwiGLU               = 1.1 e_g (|up| + e_u) + |silu(g)| e_u + u (16 + 4 |g|) |ref|,  e_g / e_u the e_pre of gate / up
  bf16 output          = the f32 bound + 1 bf16 ulp of max(|ref|, |out|)

Norms: norm_bound() below, derived in the docstring of test_gpu_norm_exact.py."""
import math

import torch

from test_gpu_decode_plan import C_DOT, U, _assert_within, _bf16_ulp  # noqa: F401  (re-exported)

GELU_SLOPE = 1.13       # sup |gelu'(x)| = 1.1290
GELU_ABS = 1.5e-6       # csrc/common.h: |gelu_erf2 - exact| <= 1.5e-6 absolute
SILU_SLOPE = 1.1        # sup |silu'(x)| = 1.0998


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
    return bound + _bf16_ulp(torch.maximum(ref.abs(), out.double().abs()))


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

"""The torch reference of the FP8 row-quantisation contract (include/icl_hip.h: icl_pack_fp8_weights, "FP8 KV cache"), shared by
test_gpu_fp8.py (weight rows), test_gpu_fp8_kv.py (cache rows), test_gpu_gqa.py / test_gpu_qknorm.py (the oracle on W') and
test_gpu_far_offsets.py.  Not a test module: plain functions over torch tensors on any device.

A row x [D] is stored as bytes q = e4m3fn(x / 2^e) and the scale 2^e, and stands for x' = q * 2^e.  With m the row's largest
magnitude and (mant, ex) = frexp(m): e = ex - 9 where mant <= 0.875, else ex - 8 (so that m / 2^e <= 448), and e = 0 for an all-zero
row.  The scaling is exact (a power of two, in float64); the rounding is torch's own e4m3fn conversion."""
import torch


def pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as float64, built from its bits (exact; torch.ldexp / exp2 on the device go through an inexact pow)."""
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def ref_q(x: torch.Tensor):
    """Rows x bf16 [..., D] (a weight matrix [N, K] is N rows) -> (bytes uint8 [..., D], scales f32 [...] = 2^e, x' bf16)."""
    xf = x.double()
    m = xf.abs().amax(-1)
    mant, ex = torch.frexp(m)
    e = torch.where(mant <= 0.875, ex - 9, ex - 8)
    e = torch.where(m == 0, torch.zeros_like(e), e)
    q = (xf * pow2(-e)[..., None]).float().to(torch.float8_e4m3fn)            # exact scaling, then torch's RNE rounding
    xp = (q.double() * pow2(e)[..., None]).to(torch.bfloat16)
    return q.view(torch.uint8), pow2(e).float(), xp


def ref_pack(q: torch.Tensor) -> torch.Tensor:
    """q [N, K] uint8 row-major -> the fp8 decode-packed layout (rows padded to 16; 16-B pieces of two 32-wide k-steps)."""
    N, K = q.shape
    Np = (N + 15) // 16 * 16
    qp = torch.zeros(Np, K, dtype=torch.uint8, device=q.device)
    qp[:N] = q
    # q[16 nt + fr][64 j + 32 h + 8 fq + i] -> piece (nt, j, lane = fq * 16 + fr), byte h * 8 + i
    return qp.view(Np // 16, 16, K // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).reshape(Np, K)


def edge_rows(D):
    """The contract's edge rows (bf16 [8, D], on the CPU): all-zero, one nonzero, amax exactly 448 * 2^e, e4m3 subnormal range,
    negative zero, ties."""
    r = torch.zeros(8, D, dtype=torch.float64)
    r[1, 5] = -3.0                                    # a single nonzero
    r[2] = torch.linspace(-1, 1, D)
    r[2, 7] = 448 * 2.0 ** -3                         # amax exactly at 448 * 2^e
    r[3] = torch.linspace(-1, 1, D) * 2.0 ** -10      # q in the e4m3 subnormal range (< 2^-6) next to the row maximum
    r[3, 0] = 448 * 2.0 ** -3
    r[4] = -0.0                                       # negative zero everywhere (amax 0: e = 0, bytes 0x80)
    r[5, ::3] = -0.0
    r[5, 1] = 1e-3
    r[6] = 448 * 2.0 ** 5 + torch.arange(D) * 2.0 ** 3    # rounding ties of the 3-bit mantissa
    r[7] = torch.randn(D, generator=torch.Generator().manual_seed(7)) * 2.0 ** 40
    return r.to(torch.bfloat16)


def w_prime_state(sd, c):
    """The checkpoint of the bf16 model that computes on W' (README's rule of the FP8 weight mode, on the CPU): the packed GEMM
    weights rounded row by row, split back out."""
    from icl_speech_text_llm_amd.runtime.packing import pack_llama, qkv_row_blocks
    w = pack_llama(dict(sd), c, "cpu")
    h, I, r = c.hidden, c.ffn, c.lora_rank
    out = dict(sd)
    for i, L in enumerate(w.layers):
        p = f"llama_model.model.layers.{i}."
        wqkv = ref_q(L.wqkv)[2].float()
        for n, (r0, nr) in zip(("q_proj", "k_proj", "v_proj"), qkv_row_blocks(c)):
            out[p + f"self_attn.{n}.weight"] = wqkv[r0:r0 + nr, :h]
            if n in c.lora_targets:
                ti = c.lora_targets.index(n)
                out[p + f"self_attn.{n}.lora_B.weight"] = wqkv[r0:r0 + nr, h + ti * r:h + (ti + 1) * r]
        gu = ref_q(L.wgu)[2].float().view(I // 16, 2, 16, h)
        out[p + "mlp.gate_proj.weight"], out[p + "mlp.up_proj.weight"] = gu[:, 0].reshape(I, h), gu[:, 1].reshape(I, h)
        out[p + "self_attn.o_proj.weight"] = ref_q(L.wo)[2].float()
        out[p + "mlp.down_proj.weight"] = ref_q(L.wdown)[2].float()
    return out

"""ctypes binding of libicl_hip.so (include/icl_hip.h).

PyTorch-ROCm is plumbing here: it owns device memory (``tensor.data_ptr()``) and the HIP stream
(``torch.cuda.current_stream().cuda_stream``); every arithmetic op of the hot path goes through the
C-ABI below.  The library is loaded from the in-tree ``lib/`` directory only; if it is missing the
import of this module fails loudly (no CPU / eager fallback exists in the product path).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_int64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libicl_hip.so"))

ICL_BF16, ICL_F32 = 0, 1
EPI_BIAS, EPI_GELU, EPI_RESIDUAL, EPI_SWIGLU = 1, 2, 4, 8
ABI_VERSION = 6
SAMPLE_TOP_K_MAX = 1024      # SAMPLE_CAP of csrc/sampling.hip: candidate-list size of icl_sample_eos


# bench.py sets this to a list to time every GEMM launch with HIP events on the launch stream:
# entries are (tile, split_k, algorithmic_flops, start_event, end_event, (M, N, K, batch))
GEMM_PROFILE = None


class IclError(RuntimeError):
    """Raised when a libicl_hip entry point returns a negative code."""


class GemmArgs(Structure):
    _fields_ = [
        ("A", c_void_p), ("W", c_void_p), ("C", c_void_p), ("bias", c_void_p), ("R", c_void_p),
        ("workspace", c_void_p),
        ("lda", c_int64), ("ldw", c_int64), ("ldc", c_int64), ("ldr", c_int64),
        ("strideA", c_int64), ("strideC", c_int64), ("strideR", c_int64),
        ("M", c_int32), ("N", c_int32), ("K", c_int32), ("batch", c_int32), ("epilogue", c_int32),
        ("out_dtype", c_int32), ("res_dtype", c_int32), ("split_k", c_int32), ("tile", c_int32),
    ]


class AttnArgs(Structure):
    _fields_ = [
        ("Q", c_void_p), ("K", c_void_p), ("V", c_void_p), ("O", c_void_p),
        ("cu_seqlens", c_void_p), ("kv_lens", c_void_p), ("rel_bias", c_void_p), ("rel_gate", c_void_p),
        ("ldq", c_int64), ("ldk", c_int64), ("ldv", c_int64), ("ldo", c_int64),
        ("n_seqs", c_int32), ("max_seqlen", c_int32), ("n_heads", c_int32), ("head_dim", c_int32),
        ("causal", c_int32), ("rel_span", c_int32), ("scale", c_float), ("n_kv_heads", c_int32),
        ("kv_seq_stride", c_int64), ("kv_head_stride", c_int64),
    ]


# icl_attn_decode_bf16 and its 16-elements-per-lane reference: Q, ldq, Kc, Vc, O, ldo, lens, n_seqs, n_heads, head_dim, max_len, scale, stream
_DECODE_PLAIN = [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p]

# name -> (restype, argtypes); mirrors include/icl_hip.h one to one
_SIGNATURES = {
    "icl_abi_version": (c_int, []),
    "icl_last_error": (c_char_p, []),
    "icl_device_cu_count": (c_int, []),
    "icl_gemm_bf16": (c_int, [POINTER(GemmArgs), c_void_p]),
    "icl_gemm_rmsnorm_bf16": (c_int, [POINTER(GemmArgs), c_void_p, c_float, c_void_p, c_int64, c_void_p]),
    "icl_gemm_select_tile": (c_int, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "icl_attn_fwd_bf16": (c_int, [POINTER(AttnArgs), c_void_p]),
    "icl_attn_fwd_suffix_bf16": (c_int, [POINTER(AttnArgs), c_void_p, c_void_p]),
    "icl_attn_decode_bf16": (c_int, _DECODE_PLAIN),
    "icl_attn_decode_gqa_bf16": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                         c_int32, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p]),
    "icl_attn_segmass_bf16": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p,
                                      c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p]),
    "icl_attn_segflow_bf16": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int32, c_int32,
                                      c_int32, c_int32, c_int32, c_int32, c_float, c_void_p]),
    "icl_attn_decode_masked_bf16": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                            c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_float,
                                            c_void_p]),
    "icl_attn_cut_tile_rows": (c_int, [c_int32, c_int32, c_int32]),
    "icl_attn_cut_rows_bf16": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                       c_float, c_void_p]),
    "icl_attn_decode_rope_bf16": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float,
                                          c_void_p]),
    "icl_layernorm": (c_int, [c_void_p, c_int64, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int64,
                              c_void_p, c_int64, c_int32, c_int32, c_float, c_int32, c_int32, c_void_p]),
    "icl_rmsnorm": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_float,
                            c_int32, c_int32, c_void_p]),
    "icl_rope_kv_bf16": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "icl_rope_kv_gqa_bf16": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "icl_qknorm_rope_kv_bf16": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                        c_void_p]),
    "icl_gemm_rope_kv_bf16": (c_int, [POINTER(GemmArgs), c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "icl_pack_decode_weights": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    "icl_pack_fp8_weights": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "icl_gemm_fp8w": (c_int, [POINTER(GemmArgs), c_void_p, c_void_p]),
    "icl_gemm_rmsnorm_fp8w": (c_int, [POINTER(GemmArgs), c_void_p, c_void_p, c_float, c_void_p, c_int64, c_void_p]),
    "icl_embed_gather_interleave": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                            c_int32, c_int32, c_void_p]),
    "icl_argmax_eos": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                               c_int32, c_int32, c_void_p, c_void_p]),
    "icl_argmax_fsm": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                               c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p,
                               c_void_p, c_void_p]),
    "icl_sample_eos": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_int32, c_int32,
                               c_float, c_float, c_int32, c_float, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                               c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p]),
    "icl_beam_step": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, c_float,
                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "icl_kv_copy_spans_bf16": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                       c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "icl_kv_copy_spans_fp8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p] + [c_int64] * 12 +
                              [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p] + [c_int32] * 9 + [c_void_p]),
    "icl_kv_append_fp8": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "icl_rope_kv_fp8": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "icl_attn_decode_bf16_epl16": (c_int, _DECODE_PLAIN),
    "icl_attn_decode_fp8": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                    c_int32, c_int32, c_int32, c_int32, c_float, c_void_p]),
    "icl_attn_decode_rope_fp8": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_int32,
                                         c_int32, c_float, c_void_p]),
    "icl_logmel_whisper": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_void_p,
                                   c_void_p, c_int64, c_void_p, c_void_p]),
    "icl_spec_to_xt": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_int64, c_void_p]),
    "icl_fbank_kaldi": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_float, c_float,
                                c_void_p, c_void_p]),
    "icl_qformer_window_xattn": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64,
                                         c_int32, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p]),
    "icl_beats_gate": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                               c_void_p]),
    "icl_axpby_cast": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_int32, c_float, c_void_p,
                               c_int64, c_int32, c_int32, c_int32, c_void_p]),
    "icl_lora_down_bf16": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_int32, c_float, c_int32,
                                   c_void_p]),
    "icl_beats_patchify": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "icl_beats_posconv_pack": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                       c_void_p]),
    "icl_gather_rows_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p]),
    "icl_gather_rows_bf16": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p]),
    "icl_cross_entropy": (c_int, [c_void_p, c_int64, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "icl_resid_rows_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_int64, c_int32,
                                   c_float, c_void_p]),
    "icl_head_rows_bf16": (c_int, [c_void_p, c_int64, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_int32,
                                   c_void_p, c_int64, c_int32, c_float, c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def load_library() -> ctypes.CDLL:
    """Load lib/libicl_hip.so (once) and type every entry point.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("ICL_LIB_PATH") or LIB_PATH        # A/B runs against another build of the same ABI
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C icl-speech-text-llm_amd/csrc`). There is no CPU fallback for the HIP path.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    ver = lib.icl_abi_version()
    if ver != ABI_VERSION:
        raise ImportError(f"libicl_hip ABI version {ver} != binding version {ABI_VERSION}")
    _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load_library().icl_last_error()
        raise IclError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")


def _eos_pair(eos_id):
    """int | (int,) | (int, int) -> (eos_id, eos_id2); -1 = unused (HF takes one id or a list; two cover the reference's models)."""
    if isinstance(eos_id, (tuple, list)):
        ids = [int(e) for e in eos_id]
        if not 1 <= len(ids) <= 2:
            raise ValueError(f"one or two EOS ids are supported, not {ids}")
        return ids[0], (ids[1] if len(ids) == 2 and ids[1] != ids[0] else -1)
    return int(eos_id), -1


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return ICL_BF16
    if t.dtype == torch.float32:
        return ICL_F32
    raise TypeError(f"unsupported dtype {t.dtype}")


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise IclError("libicl_hip operands must live on the GPU (no CPU fallback in the product path)")


# ------------------------------------------------------------------------------------------------
# thin wrappers (shapes are taken from the tensors; leading dimensions from strides)
# ------------------------------------------------------------------------------------------------
def gemm(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, bias=None, residual=None, gelu=False,
         swiglu=False, split_k: int = 1, workspace=None, tile: int = 0, M=None, K=None, lda=None,
         batch: int = 1, stride_a: int = 0, stride_c: int = 0, stride_r: int = 0, rope=None, N=None, w_scale=None) -> torch.Tensor:
    """out = epilogue(a @ w.T).  a: bf16 [M,K] (row stride lda), w: bf16 [N,K], out: bf16|f32 [M,N'].

    ``w_scale`` (f32 [N]): ``w`` is the fp8 decode-packed copy of ``pack_fp8_weights`` and the product is taken with
    W' = q * w_scale on the fp8-weight skinny kernel (icl_gemm_fp8w: M <= 64; ``tile`` is ignored, ``N`` and ``K`` are required).

    ``rope`` = (k_off, v_off, cos, sin, pos, seq_ids, kcache, vcache, n_heads, head_dim, max_len[, kv_rows_to_c]) runs the QKV projection
    with RoPE + KV-cache append fused into its epilogue (icl_gemm_rope_kv_bf16; see ``rope_fusable``)."""
    _require_gpu(a, w, out, bias, residual, workspace)
    lib = load_library()
    g = GemmArgs()
    _require_gpu(w_scale)
    N = w.shape[0] if N is None else N      # tile 5 takes the decode-packed copy (rows padded to 16): pass the true N
    g.A, g.W, g.C = a.data_ptr(), w.data_ptr(), out.data_ptr()
    g.bias, g.R, g.workspace = _ptr(bias), _ptr(residual), _ptr(workspace)
    g.lda = a.stride(-2) if lda is None else lda
    g.ldw = w.stride(0) if w_scale is None else w.shape[1]
    g.ldc = out.stride(-2)
    g.ldr = residual.stride(-2) if residual is not None else 0
    g.strideA, g.strideC, g.strideR = stride_a, stride_c, stride_r
    g.M = a.shape[-2] if M is None else M
    g.N = N
    g.K = w.shape[1] if K is None else K
    g.batch = batch
    epi = 0
    if bias is not None:
        assert bias.dtype == torch.float32
        epi |= EPI_BIAS
    if gelu:
        epi |= EPI_GELU
    if residual is not None:
        epi |= EPI_RESIDUAL
    if swiglu:
        epi |= EPI_SWIGLU
    g.epilogue = epi
    g.out_dtype = _dt(out)
    g.res_dtype = _dt(residual) if residual is not None else ICL_F32
    g.split_k = split_k
    if w_scale is not None:
        assert w.dtype == torch.uint8 and w_scale.dtype == torch.float32 and rope is None
        tile = "fp8w"                # the profiler hook's label; the library ignores args.tile here
    elif tile == 0:  # resolve the library's auto choice here so a profiler hook knows which kernel ran
        tile = lib.icl_gemm_select_tile(g.M, N, g.K, batch, split_k)
    g.tile = tile if w_scale is None else 0
    if split_k > 1 and workspace is not None:
        assert workspace.dtype == torch.float32 and workspace.numel() >= split_k * g.M * N
    if rope is not None:
        k_off, v_off, cos, sin, pos, seq_ids, kcache, vcache, n_heads, head_dim, max_len = rope[:11]
        kv_rows_to_c = int(rope[11]) if len(rope) > 11 else 1
        _require_gpu(cos, sin, pos, seq_ids, kcache, vcache)

        def launch():
            _check(lib.icl_gemm_rope_kv_bf16(ctypes.byref(g), k_off, v_off, cos.data_ptr(), sin.data_ptr(), pos.data_ptr(),
                                             _ptr(seq_ids), _ptr(kcache), _ptr(vcache), n_heads, head_dim, max_len,
                                             kv_rows_to_c, _stream()), "icl_gemm_rope_kv_bf16")
    elif w_scale is not None:
        def launch():
            _check(lib.icl_gemm_fp8w(ctypes.byref(g), w_scale.data_ptr(), _stream()), "icl_gemm_fp8w")
    else:
        def launch():
            _check(lib.icl_gemm_bf16(ctypes.byref(g), _stream()), "icl_gemm_bf16")
    if GEMM_PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        GEMM_PROFILE.append((tile, split_k, 2.0 * g.M * N * g.K * batch, e0, e1, (g.M, N, g.K, batch)))
        return out
    launch()
    return out


def gemm_rmsnorm(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, gamma: torch.Tensor, eps: float, xn: torch.Tensor, *,
                 residual=None, split_k: int = 1, workspace=None, tile: int = 0, N=None, K=None, w_scale=None) -> torch.Tensor:
    """out = residual + a @ w.T (f32) and xn[:, :N] = bf16(rmsnorm(out) * gamma): the decode form of a projection back into the
    residual stream followed by the next RMSNorm (icl_gemm_rmsnorm_bf16: with split_k > 1 one kernel reduces, adds, stores and
    normalises).  ``w_scale``: ``w`` is an fp8 decode-packed copy, as in ``gemm`` (icl_gemm_rmsnorm_fp8w)."""
    _require_gpu(a, w, out, gamma, xn, residual, workspace, w_scale)
    lib = load_library()
    g = GemmArgs()
    N = w.shape[0] if N is None else N
    g.A, g.W, g.C = a.data_ptr(), w.data_ptr(), out.data_ptr()
    g.bias, g.R, g.workspace = 0, _ptr(residual), _ptr(workspace)
    g.lda, g.ldw, g.ldc = a.stride(-2), (w.stride(0) if w_scale is None else w.shape[1]), out.stride(-2)
    g.ldr = residual.stride(-2) if residual is not None else 0
    g.strideA = g.strideC = g.strideR = 0
    g.M, g.N, g.K, g.batch = a.shape[-2], N, (w.shape[1] if K is None else K), 1
    g.epilogue = EPI_RESIDUAL if residual is not None else 0
    g.out_dtype, g.res_dtype, g.split_k = _dt(out), ICL_F32, split_k
    assert out.dtype == torch.float32 and xn.dtype == torch.bfloat16 and gamma.dtype == torch.float32
    if w_scale is not None:
        assert w.dtype == torch.uint8 and w_scale.dtype == torch.float32
        g.tile = 0
        _check(lib.icl_gemm_rmsnorm_fp8w(ctypes.byref(g), w_scale.data_ptr(), gamma.data_ptr(), eps, xn.data_ptr(), xn.stride(0),
                                         _stream()), "icl_gemm_rmsnorm_fp8w")
        return out
    g.tile = tile if tile else lib.icl_gemm_select_tile(g.M, N, g.K, 1, split_k)
    if split_k > 1 and workspace is not None:
        assert workspace.dtype == torch.float32 and workspace.numel() >= split_k * g.M * N
    _check(lib.icl_gemm_rmsnorm_bf16(ctypes.byref(g), gamma.data_ptr(), eps, xn.data_ptr(), xn.stride(0), _stream()),
           "icl_gemm_rmsnorm_bf16")
    return out


def pack_decode_weights(w: torch.Tensor, K=None) -> torch.Tensor:
    """Decode-packed copy of a row-major bf16 weight [N, >=K] for ``gemm(..., tile=5, N=N)`` (icl_pack_decode_weights)."""
    _require_gpu(w)
    assert w.dtype == torch.bfloat16 and w.dim() == 2
    N, K = w.shape[0], (w.shape[1] if K is None else K)
    out = torch.empty((N + 15) // 16 * 16, K, dtype=torch.bfloat16, device=w.device)
    _check(load_library().icl_pack_decode_weights(w.data_ptr(), w.stride(0), N, K, out.data_ptr(), _stream()),
           "icl_pack_decode_weights")
    return out


def pack_fp8_weights(w: torch.Tensor, K=None, out=None):
    """FP8 weight mode (icl_pack_fp8_weights): row-major bf16 w [N, >=K] -> (q, scales, w_deq).  q: uint8 [ceil(N/16)*16, K], the
    fp8 decode-packed copy for ``gemm(..., w_scale=scales, N=N, K=K)``; scales: f32 [N] = 2^e_n; w_deq: bf16 W' = q * 2^e_n written
    into ``out`` (``out=w`` rewrites w in place; default: a new [N, K] tensor).  Waits for the GPU: raises IclError on a NaN or an
    infinity in w."""
    _require_gpu(w, out)
    assert w.dtype == torch.bfloat16 and w.dim() == 2
    N, K = w.shape[0], (w.shape[1] if K is None else K)
    q = torch.empty((N + 15) // 16 * 16, K, dtype=torch.uint8, device=w.device)
    scales = torch.empty(N, dtype=torch.float32, device=w.device)
    if out is None:
        out = torch.empty(N, K, dtype=torch.bfloat16, device=w.device)
    assert out.dtype == torch.bfloat16 and out.shape[0] == N and out.shape[1] >= K and out.stride(1) == 1
    _check(load_library().icl_pack_fp8_weights(w.data_ptr(), w.stride(0), N, K, q.data_ptr(), scales.data_ptr(), out.data_ptr(),
                                               out.stride(0), _stream()), "icl_pack_fp8_weights")
    return q, scales, out


def rope_epilogue_ok(n_heads: int, head_dim: int, K: int) -> bool:
    """True when the 256x256 tile's fused RoPE epilogue can serve this QKV projection at all (its shape conditions; ``gemm(...,
    tile=3, rope=...)`` then runs at any M — tiles 1 - 3 sum K in the same order, so pinning the tile changes no bits)."""
    return head_dim == 128 and (n_heads * head_dim) % 256 == 0 and K >= 128


def rope_fusable(M: int, n_heads: int, head_dim: int, K: int) -> bool:
    """True when the QKV projection [M, 3*n_heads*head_dim] x K runs on the 256x256 tile with the fused RoPE epilogue."""
    hd = n_heads * head_dim
    return (rope_epilogue_ok(n_heads, head_dim, K) and
            load_library().icl_gemm_select_tile(M, 3 * hd, K, 1, 1) == 3)


def attn_fwd(q, k, v, out, cu_seqlens, max_seqlen: int, n_heads: int, head_dim: int, scale: float, *,
             causal=False, kv_lens=None, rel_bias=None, rel_gate=None, rel_span: int = 0, kv_cache_max_len: int = 0, cu_q=None,
             n_kv_heads: int = 0):
    """``kv_cache_max_len`` > 0: k / v are KV-cache tensors [n_seqs, n_heads, max_len, head_dim] (read in place).
    ``n_kv_heads`` (0 = n_heads): grouped-query attention, head_dim 128 — k / v (packed rows or cache) hold that many heads.
    ``cu_q`` (int32 [n_seqs + 1]): the suffix-query form (icl_attn_fwd_suffix_bf16) — ``q`` / ``out`` hold only the last
    cu_q[s+1] - cu_q[s] queries of each sequence, packed by ``cu_q``; ``cu_seqlens`` / ``max_seqlen`` describe k / v."""
    _require_gpu(q, k, v, out, cu_seqlens, kv_lens, rel_bias, rel_gate, cu_q)
    lib = load_library()
    a = AttnArgs()
    a.Q, a.K, a.V, a.O = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.cu_seqlens, a.kv_lens = cu_seqlens.data_ptr(), _ptr(kv_lens)
    a.rel_bias, a.rel_gate = _ptr(rel_bias), _ptr(rel_gate)
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    a.n_kv_heads = n_kv_heads
    if kv_cache_max_len > 0:
        a.ldk = a.ldv = head_dim
        a.kv_seq_stride, a.kv_head_stride = (n_kv_heads or n_heads) * kv_cache_max_len * head_dim, kv_cache_max_len * head_dim
    else:
        a.kv_seq_stride = a.kv_head_stride = 0
    a.n_seqs = cu_seqlens.numel() - 1
    a.max_seqlen, a.n_heads, a.head_dim = max_seqlen, n_heads, head_dim
    a.causal, a.rel_span, a.scale = int(causal), rel_span, scale
    assert cu_seqlens.dtype == torch.int32
    if cu_q is not None:
        assert cu_q.dtype == torch.int32 and cu_q.numel() == cu_seqlens.numel()
        _check(lib.icl_attn_fwd_suffix_bf16(ctypes.byref(a), cu_q.data_ptr(), _stream()), "icl_attn_fwd_suffix_bf16")
        return out
    _check(lib.icl_attn_fwd_bf16(ctypes.byref(a), _stream()), "icl_attn_fwd_bf16")
    return out


def _fp8_cache(kq, vq, ks, vs):
    assert kq.dtype == torch.uint8 and vq.dtype == torch.uint8 and ks.dtype == torch.float32 and vs.dtype == torch.float32


def _attn_decode(entry: str, q, out, lens, cache, *args):
    """What every decode-attention form needs.  ``args`` is the entry point's argument list up to the stream, tensors as tensors
    (None: a NULL pointer) — the kernel gets no pointer that has not been through the residency check here.  What the kernel
    assumes of every form: ``q`` (or the qkv rows) and ``out`` are bf16 rows with unit inner stride, ``lens`` is int32, ``cache``
    is (K, V) in bf16 or (K, V, K scales, V scales) in uint8 / f32 — a wrong dtype would be a garbage read on the GPU."""
    _require_gpu(*(a for a in args if isinstance(a, torch.Tensor)))
    assert q.dtype == torch.bfloat16 and out.dtype == torch.bfloat16 and q.stride(-1) == 1 and out.stride(-1) == 1
    assert lens.dtype == torch.int32
    if len(cache) == 4:
        _fp8_cache(*cache)
    else:
        assert cache[0].dtype == torch.bfloat16 and cache[1].dtype == torch.bfloat16
    _check(getattr(load_library(), entry)(*(_ptr(a) if a is None or isinstance(a, torch.Tensor) else a for a in args), _stream()),
           entry)
    return out


def attn_decode(q, kcache, vcache, out, lens, n_heads: int, head_dim: int, max_len: int, scale: float):
    return _attn_decode("icl_attn_decode_bf16", q, out, lens, (kcache, vcache),
                        q, q.stride(0), kcache, vcache, out, out.stride(0), lens, q.shape[0], n_heads, head_dim, max_len, scale)


def attn_decode_gqa(q, kcache, vcache, out, lens, n_heads: int, n_kv_heads: int, head_dim: int, max_len: int, scale: float):
    """``attn_decode`` for grouped-query attention (icl_attn_decode_gqa_bf16): q / out hold ``n_heads`` heads per row, the caches
    [n_seqs, n_kv_heads, max_len, head_dim]; every cache row is read once for the query heads that share it."""
    return _attn_decode("icl_attn_decode_gqa_bf16", q, out, lens, (kcache, vcache),
                        q, q.stride(0), kcache, vcache, out, out.stride(0), lens, q.shape[0], n_heads, n_kv_heads, head_dim, max_len, scale)


def attn_segmass(q, kcache, lens, seg, mass, n_heads: int, head_dim: int, max_len: int, scale: float, *, n_kv_heads: int = 0,
                 q_rows=None, probs=None):
    """The prompt-attention readout (icl_attn_segmass_bf16): the softmax weights of one query row per sequence over the K cache
    [n_seqs, n_kv_heads, max_len, head_dim], summed per segment.  q: bf16 rows, already rotated — row ``q_rows[b]`` (int32; None:
    row b) is sequence b's query; seg: uint8 [n_seqs, >= max_len], the segment of every key (>= n_seg: counted nowhere);
    mass: f32 [n_seqs, n_heads, n_seg] (written); probs: None, or f32 [n_seqs, n_heads, >= max_len] (row b written up to lens[b])."""
    _require_gpu(q, kcache, lens, seg, mass, q_rows, probs)
    assert lens.dtype == torch.int32 and seg.dtype == torch.uint8 and mass.dtype == torch.float32 and q.dtype == torch.bfloat16
    assert q_rows is None or q_rows.dtype == torch.int32
    n_seqs = lens.numel()
    assert seg.dim() == 2 and seg.shape[0] == n_seqs and seg.stride(1) == 1
    assert mass.is_contiguous() and mass.dim() == 3 and mass.shape[0] == n_seqs and mass.shape[1] == n_heads
    if probs is not None:
        assert probs.dtype == torch.float32 and probs.dim() == 3 and tuple(probs.shape[:2]) == (n_seqs, n_heads)
        assert probs.stride(2) == 1 and probs.stride(0) == n_heads * probs.stride(1)
    _check(load_library().icl_attn_segmass_bf16(q.data_ptr(), q.stride(0), _ptr(q_rows), kcache.data_ptr(), lens.data_ptr(),
                                                seg.data_ptr(), seg.stride(0), mass.shape[2], mass.data_ptr(), _ptr(probs),
                                                probs.stride(1) if probs is not None else 0, n_seqs, n_heads, n_kv_heads,
                                                head_dim, max_len, scale, _stream()), "icl_attn_segmass_bf16")
    return mass


def attn_segflow(q, cu, kcache, seg, flow, n_heads: int, head_dim: int, max_len: int, max_seqlen: int, scale: float, *,
                 n_kv_heads: int = 0):
    """The segment-to-segment attention flow (icl_attn_segflow_bf16): the causal softmax weights of every prompt row over the K
    cache [n_seqs, n_kv_heads, max_len, head_dim], summed by (segment of the query row, segment of the key).  q: bf16 packed rows,
    already rotated — row ``cu[b] + i`` is position i of sequence b; cu: int32 [n_seqs + 1]; seg: uint8 [n_seqs, >= max_len], the
    segment of every position (>= n_seg: summed nowhere as a query, counted in no segment as a key); flow: f32 [n_seqs, n_heads,
    n_seg, n_seg], contiguous (every element written); ``max_seqlen``: the longest sequence, at most ``max_len``."""
    _require_gpu(q, cu, kcache, seg, flow)
    assert cu.dtype == torch.int32 and seg.dtype == torch.uint8 and flow.dtype == torch.float32 and q.dtype == torch.bfloat16
    assert kcache.dtype == torch.bfloat16 and q.stride(-1) == 1 and cu.is_contiguous()
    n_seqs = cu.numel() - 1
    assert seg.dim() == 2 and seg.shape[0] == n_seqs and seg.stride(1) == 1 and kcache.shape[0] == n_seqs
    assert flow.is_contiguous() and flow.dim() == 4 and tuple(flow.shape[:2]) == (n_seqs, n_heads) and flow.shape[2] == flow.shape[3]
    _check(load_library().icl_attn_segflow_bf16(q.data_ptr(), q.stride(0), cu.data_ptr(), kcache.data_ptr(), seg.data_ptr(),
                                                seg.stride(0), flow.shape[2], flow.data_ptr(), n_seqs, n_heads, n_kv_heads, head_dim,
                                                max_len, max_seqlen, scale, _stream()), "icl_attn_segflow_bf16")
    return flow


def attn_decode_masked(q, kcache, vcache, out, lens, seg, blocked, row_seq, row_q, n_heads: int, head_dim: int, max_len: int,
                       scale: float, *, n_kv_heads: int = 0):
    """Attention knockout (icl_attn_decode_masked_bf16): ``attn_decode`` / ``attn_decode_gqa`` for the listed rows only, every key
    under a segment mask.  List entry r attends over cache sequence ``row_seq[r]`` (int32) with the query at row ``row_q[r]``
    (int32) of ``q`` (bf16, already rotated) and writes that row of ``out``; other rows of ``out`` are not written.  seg: uint8
    [n_seqs, >= max_len], the segment of every key; blocked: int32 (read as u32 bit sets) [n_listed, n_heads], bit g = that query
    head does not read segment g (ids >= 32 are never blocked); lens: int32 [n_seqs], the keys of every cache sequence."""
    assert seg.dtype == torch.uint8 and blocked.dtype == torch.int32 and row_seq.dtype == torch.int32 and row_q.dtype == torch.int32
    n_seqs, n_rows = lens.numel(), row_seq.numel()
    assert row_q.numel() == n_rows and row_seq.is_contiguous() and row_q.is_contiguous()
    assert seg.dim() == 2 and seg.shape[0] == n_seqs and seg.stride(1) == 1
    assert blocked.is_contiguous() and blocked.dim() == 2 and tuple(blocked.shape) == (n_rows, n_heads)
    assert kcache.shape[0] == n_seqs and vcache.shape[0] == n_seqs
    return _attn_decode("icl_attn_decode_masked_bf16", q, out, lens, (kcache, vcache),
                        q, q.stride(0), kcache, vcache, out, out.stride(0), lens, seg, seg.stride(0), blocked, row_seq, row_q, n_rows,
                        n_heads, n_kv_heads, head_dim, max_len, scale)


def attn_cut_tile_rows(n_heads: int, head_dim: int, n_kv_heads: int = 0) -> int:
    """Rows per tile of ``attn_cut_rows`` for a form (icl_attn_cut_tile_rows): 4 multi-head, 2 at two query heads per K/V head,
    1 from three on.  A host query, no launch; a form the kernel does not have is an ``IclError``."""
    R = load_library().icl_attn_cut_tile_rows(n_heads, n_kv_heads, head_dim)
    if R <= 0:
        raise IclError(f"icl_attn_cut_tile_rows: no row-tile form for n_heads={n_heads}, n_kv_heads={n_kv_heads}, head_dim={head_dim}")
    return R


def attn_cut_rows(q, kcache, vcache, out, seg, tile_seq, row_q, row_len, blocked, n_heads: int, head_dim: int, max_len: int,
                  scale: float, *, tile_rows: int, n_kv_heads: int = 0, head_on=None):
    """Attention cuts between prompt segments (icl_attn_cut_rows_bf16): the masked decode kernel over TILES of ``tile_rows``
    listed rows of one cache sequence.  Tile t works on cache sequence ``tile_seq[t]`` (int32 [n_tiles]); its slot e = t *
    tile_rows + r reads the query at row ``row_q[e]`` (int32 [n_tiles * tile_rows]; < 0: an empty slot) of ``q`` (bf16, already
    rotated), attends over the keys j < ``row_len[e]`` (int32) whose segment ``seg[tile_seq[t], j]`` (uint8 [n_seqs, >= max_len])
    is not a bit of ``blocked[e]`` (int32, read as a u32 bit set; ids >= 32 are never blocked), and writes that row of ``out``.
    ``head_on``: None, or uint8 [n_heads] — a query head that is off is not written.  Rows no slot lists are not written."""
    assert seg.dtype == torch.uint8 and blocked.dtype == torch.int32 and tile_seq.dtype == torch.int32 and row_q.dtype == torch.int32
    n_tiles = tile_seq.numel()
    for t in (row_q, row_len, blocked):
        assert t.is_contiguous() and t.numel() == n_tiles * tile_rows
    assert tile_seq.is_contiguous() and seg.dim() == 2 and seg.stride(1) == 1 and seg.shape[0] == kcache.shape[0] == vcache.shape[0]
    assert head_on is None or (head_on.dtype == torch.uint8 and head_on.is_contiguous() and head_on.numel() == n_heads)
    return _attn_decode("icl_attn_cut_rows_bf16", q, out, row_len, (kcache, vcache),
                        q, q.stride(0), kcache, vcache, out, out.stride(0), seg, seg.stride(0), tile_seq, row_q, row_len, blocked,
                        head_on, n_tiles, tile_rows, n_heads, n_kv_heads, head_dim, max_len, scale)


def attn_decode_rope(qkv, k_off: int, v_off: int, cos, sin, pos, seq_ids, kcache, vcache, out, lens, n_heads: int,
                     head_dim: int, max_len: int, scale: float):
    """One decode step's RoPE + cache append + attention in one launch (icl_attn_decode_rope_bf16): bit-identical to
    ``rope_kv`` followed by ``attn_decode``; ``qkv`` is left as the projection wrote it."""
    assert pos.dtype == torch.int32
    return _attn_decode("icl_attn_decode_rope_bf16", qkv, out, lens, (kcache, vcache),
                        qkv, qkv.stride(0), k_off, v_off, cos, sin, pos, seq_ids, kcache, vcache, out, out.stride(0), lens, qkv.shape[0],
                        n_heads, head_dim, max_len, scale)


def attn_decode_bf16_epl16(q, kcache, vcache, out, lens, n_heads: int, head_dim: int, max_len: int, scale: float):
    """``attn_decode`` with the fp8 kernel's lane mapping (16 elements per lane): the bf16 reference of ``attn_decode_fp8``."""
    return _attn_decode("icl_attn_decode_bf16_epl16", q, out, lens, (kcache, vcache),
                        q, q.stride(0), kcache, vcache, out, out.stride(0), lens, q.shape[0], n_heads, head_dim, max_len, scale)


def attn_decode_fp8(q, kq, vq, ks, vs, out, lens, n_heads: int, head_dim: int, max_len: int, scale: float):
    """``attn_decode`` over an FP8 KV cache (uint8 rows kq / vq, f32 row scales ks / vs): icl_attn_decode_fp8."""
    return _attn_decode("icl_attn_decode_fp8", q, out, lens, (kq, vq, ks, vs),
                        q, q.stride(0), kq, vq, ks, vs, out, out.stride(0), lens, q.shape[0], n_heads, head_dim, max_len, scale)


def attn_decode_rope_fp8(qkv, k_off: int, v_off: int, cos, sin, pos, seq_ids, kq, vq, ks, vs, out, lens, n_heads: int,
                         head_dim: int, max_len: int, scale: float):
    """``attn_decode_rope`` over an FP8 KV cache (icl_attn_decode_rope_fp8): the appended row is rounded and served rounded."""
    assert pos.dtype == torch.int32
    return _attn_decode("icl_attn_decode_rope_fp8", qkv, out, lens, (kq, vq, ks, vs),
                        qkv, qkv.stride(0), k_off, v_off, cos, sin, pos, seq_ids, kq, vq, ks, vs, out, out.stride(0), lens,
                        qkv.shape[0], n_heads, head_dim, max_len, scale)


def rope_kv_fp8(qkv, k_off: int, v_off: int, cos, sin, pos, seq_ids, kq, vq, ks, vs, n_heads: int, head_dim: int,
                max_len: int, M=None):
    """``rope_kv`` with an FP8 KV cache (icl_rope_kv_fp8): q rotated in place, the rotated k and v rounded into the cache."""
    _require_gpu(qkv, cos, sin, pos, seq_ids, kq, vq, ks, vs)
    _fp8_cache(kq, vq, ks, vs)
    M = qkv.shape[0] if M is None else M
    _check(load_library().icl_rope_kv_fp8(qkv.data_ptr(), qkv.stride(0), k_off, v_off, cos.data_ptr(), sin.data_ptr(),
                                          pos.data_ptr(), seq_ids.data_ptr(), kq.data_ptr(), vq.data_ptr(), ks.data_ptr(),
                                          vs.data_ptr(), M, n_heads, head_dim, max_len, _stream()), "icl_rope_kv_fp8")


def kv_append_fp8(qkv, k_off: int, v_off: int, pos, seq_ids, kq, vq, ks, vs, n_heads: int, head_dim: int, max_len: int, M=None):
    """Round the (already rotated) k / v blocks of M qkv rows into an FP8 KV cache at (seq_ids[m], pos[m]): icl_kv_append_fp8."""
    _require_gpu(qkv, pos, seq_ids, kq, vq, ks, vs)
    _fp8_cache(kq, vq, ks, vs)
    M = qkv.shape[0] if M is None else M
    _check(load_library().icl_kv_append_fp8(qkv.data_ptr(), qkv.stride(0), k_off, v_off, pos.data_ptr(), seq_ids.data_ptr(),
                                            kq.data_ptr(), vq.data_ptr(), ks.data_ptr(), vs.data_ptr(), M, n_heads, head_dim,
                                            max_len, _stream()), "icl_kv_append_fp8")


def layernorm(x, gamma, beta, out, eps: float, *, res=None, alpha: float = 1.0, out2=None, M=None, N=None):
    _require_gpu(x, gamma, beta, out, res, out2)
    M = x.shape[0] if M is None else M
    N = x.shape[1] if N is None else N
    if res is not None:
        assert res.dtype == x.dtype and res.stride(0) == x.stride(0)
    _check(load_library().icl_layernorm(x.data_ptr(), x.stride(0), _ptr(res), alpha, gamma.data_ptr(),
                                        beta.data_ptr(), out.data_ptr(), out.stride(0), _ptr(out2),
                                        out2.stride(0) if out2 is not None else 0, M, N, eps, _dt(x), _dt(out),
                                        _stream()), "icl_layernorm")
    return out


def rmsnorm(x, gamma, out, eps: float, *, M=None, N=None):
    _require_gpu(x, gamma, out)
    M = x.shape[0] if M is None else M
    N = x.shape[1] if N is None else N
    _check(load_library().icl_rmsnorm(x.data_ptr(), x.stride(0), gamma.data_ptr(), out.data_ptr(), out.stride(0),
                                      M, N, eps, _dt(x), _dt(out), _stream()), "icl_rmsnorm")
    return out


def rope_kv(qkv, k_off: int, v_off: int, cos, sin, pos, seq_ids, kcache, vcache, n_heads: int, head_dim: int,
            max_len: int, M=None):
    _require_gpu(qkv, cos, sin, pos, seq_ids, kcache, vcache)
    M = qkv.shape[0] if M is None else M
    _check(load_library().icl_rope_kv_bf16(qkv.data_ptr(), qkv.stride(0), k_off, v_off, cos.data_ptr(),
                                           sin.data_ptr(), pos.data_ptr(), _ptr(seq_ids), _ptr(kcache),
                                           _ptr(vcache), M, n_heads, head_dim, max_len, _stream()),
           "icl_rope_kv_bf16")


def rope_kv_gqa(qkv, k_off: int, v_off: int, cos, sin, pos, seq_ids, kcache, vcache, n_heads: int, n_kv_heads: int,
                head_dim: int, max_len: int, M=None):
    """``rope_kv`` with ``n_heads`` heads in the q block and ``n_kv_heads`` in the k / v blocks and the caches."""
    _require_gpu(qkv, cos, sin, pos, seq_ids, kcache, vcache)
    M = qkv.shape[0] if M is None else M
    _check(load_library().icl_rope_kv_gqa_bf16(qkv.data_ptr(), qkv.stride(0), k_off, v_off, cos.data_ptr(),
                                               sin.data_ptr(), pos.data_ptr(), _ptr(seq_ids), _ptr(kcache),
                                               _ptr(vcache), M, n_heads, n_kv_heads, head_dim, max_len, _stream()),
           "icl_rope_kv_gqa_bf16")


def qknorm_rope_kv(qkv, k_off: int, v_off: int, q_gamma, k_gamma, eps: float, cos, sin, pos, seq_ids, kcache, vcache,
                   n_heads: int, n_kv_heads: int, head_dim: int, max_len: int, M=None):
    """``rope_kv_gqa`` with the per-head RMSNorm of a QK-norm decoder (Qwen3) in front of the rotation: every q head row is
    normalised over ``head_dim`` with ``q_gamma``, every k head row with ``k_gamma`` (f32 [head_dim]), rounded to bf16, rotated."""
    _require_gpu(qkv, q_gamma, k_gamma, cos, sin, pos, seq_ids, kcache, vcache)
    M = qkv.shape[0] if M is None else M
    _check(load_library().icl_qknorm_rope_kv_bf16(qkv.data_ptr(), qkv.stride(0), k_off, v_off, _ptr(q_gamma), _ptr(k_gamma),
                                                  eps, cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), _ptr(seq_ids),
                                                  _ptr(kcache), _ptr(vcache), M, n_heads, n_kv_heads, head_dim, max_len,
                                                  _stream()),
           "icl_qknorm_rope_kv_bf16")


def embed_gather_interleave(src_idx, table, speech, out):
    _require_gpu(src_idx, table, speech, out)
    assert src_idx.dtype == torch.int32 and table.dtype == torch.bfloat16 and out.dtype == torch.float32
    _check(load_library().icl_embed_gather_interleave(src_idx.data_ptr(), table.data_ptr(), _ptr(speech),
                                                      out.data_ptr(), src_idx.numel(), table.shape[1],
                                                      table.shape[0], 0 if speech is None else speech.shape[0],
                                                      _stream()), "icl_embed_gather_interleave")
    return out


def argmax_eos(logits, eos_id, pad_id: int, finished, out_tokens, step: int, next_ids, V=None):
    _require_gpu(logits, finished, out_tokens, next_ids)
    e1, e2 = _eos_pair(eos_id)
    _check(load_library().icl_argmax_eos(logits.data_ptr(), logits.stride(0), logits.shape[0],
                                         logits.shape[1] if V is None else V, e1, e2, pad_id, finished.data_ptr(),
                                         out_tokens.data_ptr(), out_tokens.stride(0), step, next_ids.data_ptr(),
                                         _stream()), "icl_argmax_eos")


def argmax_fsm(logits, tables, state, steps_left: int, eos_id, pad_id: int, finished, out_tokens, step: int, next_ids,
               out_logprob=None, V=None):
    """Constrained greedy decode tail (icl_argmax_fsm).  ``tables`` = the device copy of a ``constraints.LabelAutomaton``
    (``.state_off`` / ``.edge_tok`` / ``.edge_next`` / ``.state_dist`` int32, ``.n_states``, ``.n_edges``, ``.vocab``); ``state``
    int32 [B] holds each row's state (-1 = free row) and is advanced in place; ``out_logprob`` f32 shaped like ``out_tokens``."""
    _require_gpu(logits, tables.state_off, tables.edge_tok, tables.edge_next, tables.state_dist, state, finished, out_tokens,
                 next_ids, out_logprob)
    V = logits.shape[1] if V is None else V
    if tables.vocab > V:           # the kernel reads logits[b][edge_tok[e]]: an automaton over a larger vocabulary is a caller's error
        raise ValueError(f"automaton built for a vocabulary of {tables.vocab} ids used on logits of {V}")
    assert logits.dtype == torch.float32 and state.dtype == torch.int32 and state.numel() == logits.shape[0]
    assert out_logprob is None or (out_logprob.dtype == torch.float32 and out_logprob.stride(0) == out_tokens.stride(0))
    e1, e2 = _eos_pair(eos_id)
    _check(load_library().icl_argmax_fsm(logits.data_ptr(), logits.stride(0), logits.shape[0], V, tables.state_off.data_ptr(),
                                         tables.edge_tok.data_ptr(), tables.edge_next.data_ptr(), tables.state_dist.data_ptr(),
                                         tables.n_states, tables.n_edges, state.data_ptr(), steps_left, e1, e2, pad_id,
                                         finished.data_ptr(), out_tokens.data_ptr(), out_tokens.stride(0), step,
                                         next_ids.data_ptr(), _ptr(out_logprob), _stream()), "icl_argmax_fsm")


def sample_eos(logits, work, uniforms, eos_id, pad_id: int, finished, out_tokens, step: int, next_ids, *,
               temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0, repetition_penalty: float = 1.0, V=None,
               debug=None):
    """Sampled decode tail: tokens generated so far (``out_tokens[:, :step]``) feed the repetition penalty; ``uniforms`` f32 [B]
    are the draws; ``debug`` = (ids int32 [B,cap], probs f32 [B,cap], count int32 [B]) receives the kept distribution."""
    _require_gpu(logits, work, uniforms, finished, out_tokens, next_ids)
    assert logits.dtype == torch.float32 and work.dtype == torch.float32 and uniforms.dtype == torch.float32
    V = logits.shape[1] if V is None else V
    e1, e2 = _eos_pair(eos_id)
    dbg = (None, None, None, 0)
    if debug is not None:
        _require_gpu(*debug)
        dbg = (debug[0].data_ptr(), debug[1].data_ptr(), debug[2].data_ptr(), debug[0].shape[1])
    _check(load_library().icl_sample_eos(logits.data_ptr(), logits.stride(0), logits.shape[0], V, work.data_ptr(),
                                         work.stride(0), out_tokens.data_ptr(), out_tokens.stride(0), step,
                                         repetition_penalty, temperature, top_k, top_p, uniforms.data_ptr(), e1, e2, pad_id,
                                         finished.data_ptr(), out_tokens.data_ptr(), out_tokens.stride(0), step,
                                         next_ids.data_ptr(), dbg[0], dbg[1], dbg[2], dbg[3], _stream()), "icl_sample_eos")


class BeamState:
    """Device-resident state of ``icl_beam_step`` for B rows x K beams x T new tokens (see include/icl_hip.h)."""

    def __init__(self, get, B: int, K: int, T: int, pad_id: int):
        f32, i32 = torch.float32, torch.int32
        self.B, self.K, self.T = B, K, T
        self.run_score, self.fin_score = get("gen_beam_run_score", (B, K), f32), get("gen_beam_fin_score", (B, K), f32)
        self.run_seq, self.fin_seq = get("gen_beam_run_seq", (B, K, T), i32), get("gen_beam_fin_seq", (B, K, T), i32)
        self.fin_len, self.fin_flag = get("gen_beam_fin_len", (B, K), i32), get("gen_beam_fin_flag", (B, K), i32)
        self.unsat = get("gen_beam_unsat", (B,), i32)
        self.next_ids, self.parent = get("gen_beam_next", (B * K,), i32), get("gen_beam_parent", (B * K,), i32)
        self.run_score.fill_(-1.0e9)
        self.run_score[:, 0] = 0.0
        self.fin_score.fill_(-1.0e9)
        self.run_seq.fill_(pad_id)
        self.fin_seq.fill_(pad_id)
        self.fin_len.zero_()
        self.fin_flag.zero_()
        self.unsat.fill_(1)


def beam_step(logits, state: BeamState, step: int, eos_id, length_penalty: float, V=None, repetition_penalty: float = 1.0):
    """One beam-search step over ``logits`` f32 [B, V] (step 0: the prompt's distribution, shared by the K beams) or
    [B * K, V] (row b * K + k = running beam k of row b)."""
    _require_gpu(logits, state.run_score)
    assert logits.dtype == torch.float32 and logits.stride(1) == 1
    rows = logits.shape[0] // state.B
    assert rows * state.B == logits.shape[0] and rows in (1, state.K)
    e1, e2 = _eos_pair(eos_id)
    _check(load_library().icl_beam_step(logits.data_ptr(), logits.stride(0), rows, state.B,
                                        logits.shape[1] if V is None else V, state.K, state.T, step, e1, e2,
                                        float(length_penalty), float(repetition_penalty), state.run_score.data_ptr(),
                                        state.run_seq.data_ptr(),
                                        state.fin_score.data_ptr(), state.fin_seq.data_ptr(), state.fin_len.data_ptr(),
                                        state.fin_flag.data_ptr(), state.unsat.data_ptr(), state.next_ids.data_ptr(),
                                        state.parent.data_ptr(), _stream()), "icl_beam_step")


def kv_copy_spans(src, dst, n_rows: int, *, src_seq=None, src_t0=None, dst_seq=None, dst_t0=None, n_t=None, n_fixed: int = 0,
                  src_scale=None, dst_scale=None):
    """src / dst: bf16 [layers][seqs][heads][positions][head_dim] (any strides on the first three dims); copies, per row r,
    layer and head, ``n_t[r]`` (or ``n_fixed``) positions from (src_seq[r], src_t0[r]) to (dst_seq[r], dst_t0[r]).
    FP8 KV cache: src / dst are the uint8 row bytes and ``src_scale`` / ``dst_scale`` their f32 [layers][seqs][heads][positions]
    scale planes (icl_kv_copy_spans_fp8 moves both)."""
    _require_gpu(src, dst, src_seq, src_t0, dst_seq, dst_t0, n_t, src_scale, dst_scale)
    fp8 = src.dtype == torch.uint8
    assert src.dtype == dst.dtype and src.dtype in (torch.bfloat16, torch.uint8) and src.dim() == 5 and dst.dim() == 5
    assert src.stride(4) == 1 and dst.stride(4) == 1 and src.stride(3) == src.shape[4] and dst.stride(3) == dst.shape[4]
    assert src.shape[0] == dst.shape[0] and src.shape[2] == dst.shape[2] and src.shape[4] == dst.shape[4]
    for t in (src_seq, src_t0, dst_seq, dst_t0, n_t):
        assert t is None or (t.dtype == torch.int32 and t.numel() >= n_rows)
    ids = (_ptr(src_seq), _ptr(src_t0), _ptr(dst_seq), _ptr(dst_t0), _ptr(n_t), n_fixed, n_rows, src.shape[0], src.shape[2],
           src.shape[4], src.shape[1], dst.shape[1], src.shape[3], dst.shape[3], _stream())
    if fp8:
        assert src_scale is not None and dst_scale is not None and src_scale.dtype == torch.float32 and dst_scale.dtype == torch.float32
        assert tuple(src_scale.shape) == tuple(src.shape[:4]) and tuple(dst_scale.shape) == tuple(dst.shape[:4])
        assert src_scale.stride(3) == 1 and dst_scale.stride(3) == 1
        _check(load_library().icl_kv_copy_spans_fp8(src.data_ptr(), src_scale.data_ptr(), dst.data_ptr(), dst_scale.data_ptr(),
                                                    src.stride(0), src.stride(1), src.stride(2), dst.stride(0), dst.stride(1),
                                                    dst.stride(2), src_scale.stride(0), src_scale.stride(1), src_scale.stride(2),
                                                    dst_scale.stride(0), dst_scale.stride(1), dst_scale.stride(2), *ids),
               "icl_kv_copy_spans_fp8")
        return
    assert src_scale is None and dst_scale is None
    _check(load_library().icl_kv_copy_spans_bf16(src.data_ptr(), dst.data_ptr(), src.stride(0), src.stride(1), src.stride(2),
                                                 dst.stride(0), dst.stride(1), dst.stride(2), *ids), "icl_kv_copy_spans_bf16")


def logmel_whisper(wav, wav_lens, mel_filters, n_mel: int, spec, xt, workspace):
    _require_gpu(wav, wav_lens, mel_filters, spec, xt, workspace)
    assert wav.dtype == torch.float32 and mel_filters.dtype == torch.float64 and wav_lens.dtype == torch.int32
    _check(load_library().icl_logmel_whisper(wav.data_ptr(), wav.stride(0), wav_lens.data_ptr(),
                                             mel_filters.data_ptr(), n_mel, wav.shape[0], _ptr(spec), _ptr(xt),
                                             xt.stride(-2) if xt is not None else 0, workspace.data_ptr(),
                                             _stream()), "icl_logmel_whisper")


def spec_to_xt(spec, xt):
    _require_gpu(spec, xt)
    assert spec.dtype == torch.float32 and spec.is_contiguous()
    _check(load_library().icl_spec_to_xt(spec.data_ptr(), spec.shape[1], spec.shape[0], xt.data_ptr(),
                                         xt.stride(-2), _stream()), "icl_spec_to_xt")


def fbank_kaldi(wav, wav_lens, mel_banks, max_frames: int, mean: float, std: float, out):
    _require_gpu(wav, wav_lens, mel_banks, out)
    assert wav.dtype == torch.float32 and mel_banks.dtype == torch.float64 and wav_lens.dtype == torch.int32
    _check(load_library().icl_fbank_kaldi(wav.data_ptr(), wav.stride(0), wav_lens.data_ptr(), mel_banks.data_ptr(),
                                          wav.shape[0], max_frames, mean, std, out.data_ptr(), _stream()),
           "icl_fbank_kaldi")


def qformer_window_xattn(q, kv, v_off: int, out, n_audio: int, win_per_audio: int, win: int, rows_per_audio: int,
                         n_heads: int, scale: float):
    _require_gpu(q, kv, out)
    _check(load_library().icl_qformer_window_xattn(q.data_ptr(), q.stride(0), kv.data_ptr(), kv.stride(0), v_off,
                                                   out.data_ptr(), out.stride(0), n_audio, win_per_audio, win,
                                                   rows_per_audio, n_heads, scale, _stream()),
           "icl_qformer_window_xattn")


def beats_gate(qkv, grep_w, grep_b, grep_a, gate, n_heads: int, M=None):
    _require_gpu(qkv, grep_w, grep_b, grep_a, gate)
    M = qkv.shape[0] if M is None else M
    _check(load_library().icl_beats_gate(qkv.data_ptr(), qkv.stride(0), grep_w.data_ptr(), grep_b.data_ptr(),
                                         grep_a.data_ptr(), gate.data_ptr(), M, n_heads, _stream()),
           "icl_beats_gate")


def axpby_cast(x, out, alpha: float = 1.0, add=None):
    _require_gpu(x, out, add)
    M, N = x.shape
    _check(load_library().icl_axpby_cast(x.data_ptr(), x.stride(0), _dt(x), _ptr(add),
                                         add.stride(0) if add is not None else 0,
                                         _dt(add) if add is not None else ICL_F32, alpha, out.data_ptr(),
                                         out.stride(0), _dt(out), M, N, _stream()), "icl_axpby_cast")
    return out


def lora_down(x, K0: int, a, r_total: int, scale: float, M=None):
    _require_gpu(x, a)
    M = x.shape[0] if M is None else M
    _check(load_library().icl_lora_down_bf16(x.data_ptr(), x.stride(0), K0, a.data_ptr(), a.stride(0), r_total,
                                             scale, M, _stream()), "icl_lora_down_bf16")


def device_cu_count() -> int:
    return load_library().icl_device_cu_count()


def beats_patchify(fbank, cu_rows, total_rows: int, out):
    _require_gpu(fbank, cu_rows, out)
    _check(load_library().icl_beats_patchify(fbank.data_ptr(), fbank.shape[1], cu_rows.data_ptr(), fbank.shape[0],
                                             total_rows, out.data_ptr(), _stream()), "icl_beats_patchify")


def beats_posconv_pack(x, cu_rows, valid_rows, n_audio: int, total_rows: int, groups: int, xg):
    _require_gpu(x, cu_rows, valid_rows, xg)
    _check(load_library().icl_beats_posconv_pack(x.data_ptr(), cu_rows.data_ptr(), valid_rows.data_ptr(), n_audio,
                                                 total_rows, x.shape[1], groups, xg.data_ptr(), _stream()),
           "icl_beats_posconv_pack")


def gather_rows(src, idx, out, N=None):
    """out[r, :N] = src[idx[r], :N]; f32 or bf16 (both tensors alike)."""
    _require_gpu(src, idx, out)
    assert src.dtype == out.dtype and src.dtype in (torch.float32, torch.bfloat16) and idx.dtype == torch.int32
    lib = load_library()
    fn, what = ((lib.icl_gather_rows_f32, "icl_gather_rows_f32") if src.dtype == torch.float32 else
                (lib.icl_gather_rows_bf16, "icl_gather_rows_bf16"))
    _check(fn(src.data_ptr(), src.stride(0), idx.data_ptr(), out.data_ptr(), out.stride(0), idx.numel(),
              src.shape[1] if N is None else N, _stream()), what)
    return out


RESID_MODES = {"replace": 0, "add": 1}


def resid_rows(h, rows, *, capture=None, vec=None, mode="replace", alpha: float = 1.0, hidden=None):
    """Residual-stream capture and patch at the listed rows (icl_resid_rows_f32).  h: f32 [R, >= hidden] (row stride = its
    leading dimension), patched in place; rows: int32 [n], distinct rows of h; capture: None or f32 [n, >= hidden], receives the
    rows' PRE-patch bits; vec: None or f32 [n, >= hidden] (one vector per entry) or [1, hidden] / [hidden] (one for all entries);
    mode "replace" (bits) or "add" (h = fma(alpha, vec, h), one rounding).  ``hidden``: the columns worked on (default: h's width)."""
    _require_gpu(h, rows, capture, vec)
    assert h.dtype == torch.float32 and h.dim() == 2 and h.stride(1) == 1 and rows.dtype == torch.int32 and rows.is_contiguous()
    n = rows.numel()
    hidden = h.shape[1] if hidden is None else hidden
    ld_cap = ld_vec = 0
    if capture is not None:
        assert capture.dtype == torch.float32 and capture.dim() == 2 and capture.shape[0] == n and capture.stride(1) == 1
        ld_cap = capture.stride(0)
    if vec is not None:
        assert vec.dtype == torch.float32 and vec.dim() in (1, 2) and vec.stride(-1) == 1
        assert vec.dim() == 1 or vec.shape[0] in (1, n), f"{vec.shape[0]} vectors for {n} rows"
        ld_vec = vec.stride(0) if vec.dim() == 2 and vec.shape[0] > 1 else 0      # 0: the one vector serves every entry
    mode_i = RESID_MODES[mode] if mode in RESID_MODES else int(mode)   # an integer goes through: the entry point refuses a bad one
    _check(load_library().icl_resid_rows_f32(h.data_ptr(), h.stride(0), rows.data_ptr(), n, hidden, _ptr(capture), ld_cap,
                                             _ptr(vec), ld_vec, mode_i, float(alpha), _stream()), "icl_resid_rows_f32")
    return h


def head_rows(att, rows, *, n_heads: int, head_dim: int, capture=None, heads=None, vec=None, mode="replace", alpha: float = 1.0):
    """Attention-head output capture and patch at the listed rows (icl_head_rows_bf16).  att: bf16 [R, >= n_heads * head_dim] (row
    stride = its leading dimension), patched in place; rows: int32 [n], distinct rows of att; capture: None or bf16 [n, >= n_heads *
    head_dim], receives the rows' PRE-patch bits; heads: int32 [n_sel], distinct heads; vec: None or f32 [n, n_sel, head_dim] (one
    block of vectors per entry) or [1, n_sel, head_dim] / [n_sel, head_dim] (one for all entries), in the order of ``heads``; mode
    "replace" (att = bf16(vec)) or "add" (att = bf16(fma(alpha, vec, att)))."""
    _require_gpu(att, rows, capture, heads, vec)
    assert att.dtype == torch.bfloat16 and att.dim() == 2 and att.stride(1) == 1 and rows.dtype == torch.int32 and rows.is_contiguous()
    n, n_sel = rows.numel(), 0
    ld_cap = ld_vec = 0
    if capture is not None:
        assert capture.dtype == torch.bfloat16 and capture.dim() == 2 and capture.shape[0] == n and capture.stride(1) == 1
        ld_cap = capture.stride(0)
    if heads is not None:
        assert heads.dtype == torch.int32 and heads.dim() == 1 and heads.is_contiguous()
        n_sel = heads.numel()
    if vec is not None:
        assert heads is not None, "vec needs heads"
        assert vec.dtype == torch.float32 and vec.dim() in (2, 3) and vec.shape[-2:] == (n_sel, head_dim) and vec[0].is_contiguous()
        assert vec.dim() == 2 or vec.shape[0] in (1, n), f"{vec.shape[0]} blocks of vectors for {n} rows"
        ld_vec = vec.stride(0) if vec.dim() == 3 and vec.shape[0] > 1 else 0      # 0: the one block serves every entry
    mode_i = RESID_MODES[mode] if mode in RESID_MODES else int(mode)   # an integer goes through: the entry point refuses a bad one
    _check(load_library().icl_head_rows_bf16(att.data_ptr(), att.stride(0), rows.data_ptr(), n, n_heads, head_dim, _ptr(capture),
                                             ld_cap, _ptr(heads), n_sel, _ptr(vec), ld_vec, mode_i, float(alpha), _stream()),
           "icl_head_rows_bf16")
    return att


def cross_entropy(logits, labels, row_loss, mean_loss, V=None):
    _require_gpu(logits, labels, row_loss, mean_loss)
    assert logits.dtype == torch.float32 and labels.dtype == torch.int32
    _check(load_library().icl_cross_entropy(logits.data_ptr(), logits.stride(0), labels.data_ptr(), labels.numel(),
                                            logits.shape[1] if V is None else V, row_loss.data_ptr(),
                                            mean_loss.data_ptr(), _stream()), "icl_cross_entropy")
    return mean_loss

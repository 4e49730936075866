"""Where the operands of tests/test_gpu_far_offsets.py sit: pure Python, no GPU.

Every far-offset case runs one entry point on operands that are views into one arena of ARENA_BYTES bytes.  An operand (Op) is a
pointer (arena + base) and the logical rows the launch touches, each a run of `n` elements at an element offset from that
pointer; `offs` are the offsets of the far launch, `twin` those of the compact twin launch (same values, small tensors).  A row is
FAR when its offset is at least 2^32 elements of the operand's own type.  The three forms (the issue's names):

  stride form     two logical rows, leading dimension LD_FAR = 2^32 + 64: row 1 starts at element 2^32 + 64
  index form      a device index array holds near ids and ids whose row starts beyond 2^32 elements
  grid-walk form  the index is a block id: about 1030 sequences of 2^22 elements each; offsets in [2^31, 2^32) occur too

A narrowing is what a kernel (or the binding) would compute if one 32-bit type slipped into its address arithmetic: the element
index or the byte offset, taken as int32 or as uint32 (NARROWINGS).  The layout guarantees, and tests/test_far_layout.py asserts
for every row of every case, that each narrowing of each row still lies inside the arena and inside a window the GPU test
compares, so a narrowing shows as a wrong value, never as a memory fault.

A compared window is a row, or the place one of its narrowings lands, with MARGIN bytes on either side; windows of one operand
are merged, windows of different operands never overlap.  `emulate` is the CPU model of a launch (out row i = the sum of the
input rows i, plus one) over a sparse dict of those windows, with one operand's addresses narrowed; `verdict` applies the GPU
test's three assertions to it.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import zlib

import numpy as np

ARENA_BYTES = 2 ** 34 + 2 ** 28          # 16.25 GiB: an f32 operand needs element offsets >= 2^32, i.e. 16 GiB
MARGIN = 1 << 16                         # sentinel bytes around every compared region
FAR = 1 << 32
LD_FAR = FAR + 64                        # the stride form's leading dimension; every narrowing of it is 64
SLOT = 64 << 20                          # spacing of the operands' bases, so that equal indices do not collide
FIRST_BASE = 1 << 20
ESIZE = {"f32": 4, "bf16": 2, "u8": 1, "i32": 4}
NARROWINGS = ("elem_i32", "elem_u32", "byte_i32", "byte_u32")
SENTINEL = 0xA5


def _s32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def narrow(off, esize, kind):
    """Byte offset, from the operand's pointer, that element offset `off` becomes under narrowing `kind`."""
    if kind == "elem_i32":
        return _s32(off) * esize
    if kind == "elem_u32":
        return (off & 0xFFFFFFFF) * esize
    if kind == "byte_i32":
        return _s32(off * esize)
    if kind == "byte_u32":
        return (off * esize) & 0xFFFFFFFF
    assert kind is None
    return off * esize


@dataclass
class Op:
    name: str
    dtype: str                 # key of ESIZE
    role: str                  # "in" | "out" | "inout"
    n: int                     # elements per row
    offs: tuple                # element offsets of the rows, far launch
    twin: tuple                # element offsets of the same rows, compact twin
    low: int = 0               # bytes the operand needs below its pointer (grid-walk: a negative int32 index lands there)
    base: int = -1             # byte offset of the pointer in the arena (set by place())
    meta: dict = field(default_factory=dict)

    @property
    def esize(self):
        return ESIZE[self.dtype]

    def is_far(self):
        return any(o >= FAR for o in self.offs)

    def landings(self, offs=None):
        """Byte offsets (from the pointer) where a row can be addressed: the true place and every narrowing of it."""
        offs = self.offs if offs is None else offs
        return sorted({narrow(o, self.esize, k) for o in offs for k in (None,) + NARROWINGS})

    def windows(self, offs=None, margin=MARGIN):
        """Merged compared windows [(lo, hi)) in bytes from the pointer: every landing of every row, MARGIN on either side."""
        nb = self.n * self.esize
        out = []
        for lo in self.landings(offs):
            lo, hi = lo - margin, lo + nb + margin
            if out and lo <= out[-1][1]:
                out[-1][1] = max(out[-1][1], hi)
            else:
                out.append([lo, hi])
        return [tuple(w) for w in out]

    def expected(self, offs=None):
        """Byte ranges the launch is expected to write: the rows of an out / inout operand."""
        if self.role == "in":
            return []
        nb = self.n * self.esize
        return [(o * self.esize, o * self.esize + nb) for o in (self.offs if offs is None else offs)]


@dataclass
class Case:
    name: str
    group: str
    form: str                  # "stride" | "index" | "grid" | combinations, for the report
    ops: list
    p: dict = field(default_factory=dict)      # shape parameters of the launch

    def op(self, name):
        return next(o for o in self.ops if o.name == name)


def place(case):
    """Give every operand its base: the operands that reach furthest get the lowest bases, SLOT apart."""
    order = sorted(case.ops, key=lambda o: -(max(o.offs) * o.esize))
    base = FIRST_BASE
    for o in order:
        o.base = base
        base += SLOT + (3 << 20)          # + 3 MiB: an fp8 scale plane's far-id rows sit at multiples of 128 MiB from its base
    return case


def compact_ld(n):
    """Leading dimension of a stride-form twin: a multiple of 64 like LD_FAR (same ld % 8, same alignment of every row)."""
    return (n + 63) // 64 * 64 + 64


def stride_op(name, dtype, role, n, rows=2, **meta):
    return Op(name, dtype, role, n, tuple(r * LD_FAR for r in range(rows)), tuple(r * compact_ld(n) for r in range(rows)),
              meta=dict(meta, ld=LD_FAR, ld_twin=compact_ld(n)))


def plain_op(name, dtype, role, n, rows, ld=None, **meta):
    """An operand that stays near: the same compact rows in both launches (its neighbours are the far ones)."""
    ld = compact_ld(n) if ld is None else ld
    offs = tuple(r * ld for r in range(rows))
    return Op(name, dtype, role, n, offs, offs, meta=dict(meta, ld=ld, ld_twin=ld))


def index_op(name, dtype, role, n, row_elems, ids, **meta):
    """Rows of `row_elems` elements picked by id (n <= row_elems are touched); the twin renumbers them 0, 1, 2, ..."""
    twin_ids = tuple(range(len(ids)))
    return Op(name, dtype, role, n, tuple(i * row_elems for i in ids), tuple(i * row_elems for i in twin_ids),
              meta=dict(meta, ids=tuple(ids), ids_twin=twin_ids, row_elems=row_elems))


# ------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------
def _norm_cases():
    out = []
    for name, rms, N, in_dt, out_dt, res, y2 in (
            ("rmsnorm_n4096", True, 4096, "f32", "bf16", False, False),           # norm_kernel<true, 16>
            ("rmsnorm_n1280_stream", True, 1280, "f32", "bf16", False, False),    # norm8_kernel<true, 3>
            ("rmsnorm_bf16_n4096", True, 4096, "bf16", "bf16", False, False),
            ("layernorm_n1280_stream", False, 1280, "f32", "bf16", False, False),  # norm8_kernel<false, 3>
            ("layernorm_n4096", False, 4096, "f32", "f32", False, False),         # norm_kernel<false, 16>
            ("layernorm_res_out2_n1280", False, 1280, "f32", "f32", True, True),  # norm_kernel<false, 5>, res + y2
            ("layernorm_res_out2_n4096", False, 4096, "f32", "f32", True, True)):
        ops = [stride_op("x", in_dt, "in", N), stride_op("y", out_dt, "out", N)]
        if res:
            ops.append(stride_op("res", in_dt, "in", N))
        if y2:
            ops.append(stride_op("y2", "bf16", "out", N))
        out.append(Case(name, "norm", "stride", ops, dict(rms=rms, N=N)))
    return out


ROPE_H, ROPE_MAXLEN = 2, 64
ROPE_SIDS = (262147, 1)                     # a sequence is 2 heads x 64 positions x 128 = 2^14 elements: ids >= 2^18 start beyond
ROPE_POS = (5, 63)                          # 2^32 elements; 262147 narrows onto sequence 3.  Row 0: near qkv row, far cache row;
#                                             row 1 (qkv element 2^32 + 64): far qkv row, near cache row.


def _rope_cases():
    """Stride + index: the two qkv rows at LD_FAR, one near and one far sequence id.  *_many_ids: compact qkv rows and only the
    index far, with several near and several far ids; the fp8 byte planes (one-byte elements) reach 2^32 k + d for k = 1, 2, 3,
    so a narrowing to 33 - 40 bits shows there too (a bf16 plane of k = 2 is outside the arena)."""
    out = []
    many16, many8 = (0, 2, 262147, 262150), (1, 5, 262147, 524290, 786437)
    for name, entry, H, Hkv, D, fp8, sids, pos in (
            ("rope_kv", "rope_kv", ROPE_H, ROPE_H, 128, False, ROPE_SIDS, ROPE_POS),
            ("rope_kv_gqa", "rope_kv_gqa", 4, ROPE_H, 128, False, ROPE_SIDS, ROPE_POS),
            ("qknorm_rope_kv", "qknorm_rope_kv", 4, ROPE_H, 128, False, ROPE_SIDS, ROPE_POS),
            ("rope_kv_fp8", "rope_kv_fp8", ROPE_H, ROPE_H, 128, True, ROPE_SIDS, ROPE_POS),
            ("kv_append_fp8", "kv_append_fp8", ROPE_H, ROPE_H, 128, True, ROPE_SIDS, ROPE_POS),
            ("rope_kv_many_ids", "rope_kv", ROPE_H, ROPE_H, 128, False, many16, (5, 63, 0, 17)),
            ("kv_append_fp8_many_ids", "kv_append_fp8", ROPE_H, ROPE_H, 128, True, many8, (5, 63, 0, 17, 40))):
        M = len(sids)
        width = (H + 2 * Hkv) * D
        role = "in" if entry == "kv_append_fp8" else "inout"
        qkv = stride_op("qkv", "bf16", role, width) if M == 2 else plain_op("qkv", "bf16", role, width, M)
        seq_elems = Hkv * ROPE_MAXLEN * D

        def rows(ids):
            return tuple(s * seq_elems + h * ROPE_MAXLEN * D + p * D for s, p in zip(ids, pos) for h in range(Hkv))
        twin_ids = tuple(range(M))
        ops = [qkv]
        for c in ("kc", "vc"):
            ops.append(Op(c, "u8" if fp8 else "bf16", "out", D, rows(sids), rows(twin_ids), meta=dict(ids=sids, ids_twin=twin_ids)))
        if fp8:         # the f32 scale planes: one element per cache row, at the row's own index (not far: see the module docstring
            def srows(ids):   # of the GPU test); a narrowed plane index still lands in a compared window
                return tuple((s * Hkv + h) * ROPE_MAXLEN + p for s, p in zip(ids, pos) for h in range(Hkv))
            for c in ("ks", "vs"):
                ops.append(Op(c, "f32", "out", 1, srows(sids), srows(twin_ids)))
        out.append(Case(name, "rope", "stride (qkv) + index (cache)" if M == 2 else "index (cache)", ops,
                        dict(entry=entry, H=H, Hkv=Hkv, D=D, M=M, fp8=fp8, pos=pos)))
    return out


GATHER_IDS = (3, 1048577)    # rows of 4096 elements: ids >= 2^20 start beyond 2^32 elements


def _glue_cases():
    out = []
    for dt in ("f32", "bf16"):
        N = 4096
        out.append(Case(f"gather_rows_{dt}", "glue", "index (src) + stride (out)",
                        [index_op("src", dt, "in", N, N, GATHER_IDS), stride_op("out", dt, "out", N, rows=len(GATHER_IDS))],
                        dict(N=N)))
    for in_dt, add_dt, out_dt in (("f32", "bf16", "bf16"), ("bf16", "f32", "f32")):
        N = 200
        out.append(Case(f"axpby_cast_{in_dt}_{add_dt}_{out_dt}", "glue", "stride",
                        [stride_op("x", in_dt, "in", N), stride_op("add", add_dt, "in", N), stride_op("out", out_dt, "out", N)],
                        dict(N=N)))
    H = 4096
    out.append(Case("embed_gather_interleave", "glue", "index (table, speech)",
                    [index_op("table", "bf16", "in", H, H, (0, 7, 1048577, 1048580)),
                     index_op("speech", "f32", "in", H, H, (0, 2, 1048577, 1048581)),
                     plain_op("out", "f32", "out", H, 8, ld=H)],
                    dict(H=H, order=(("table", 0), ("speech", 2), ("table", 2), ("speech", 0), ("table", 3), ("speech", 3),
                                     ("table", 1), ("speech", 1)))))
    K0, r = 512, 16
    out.append(Case("lora_down", "glue", "stride (X)", [stride_op("x", "bf16", "inout", K0 + r),
                                                         plain_op("a", "bf16", "in", K0, r)], dict(K0=K0, r=r)))
    Hb = 12
    out.append(Case("beats_gate", "glue", "stride (qkv)", [stride_op("qkv", "bf16", "in", Hb * 64),
                                                           plain_op("gate", "f32", "out", Hb, 2, ld=Hb)], dict(H=Hb)))
    return out


def _tail_cases():
    V = 257
    out = [Case("argmax_eos", "tail", "stride (logits)", [stride_op("logits", "f32", "in", V)], dict(V=V)),
           Case("cross_entropy", "tail", "stride (logits)", [stride_op("logits", "f32", "in", V)], dict(V=V)),
           Case("argmax_fsm", "tail", "stride (logits)", [stride_op("logits", "f32", "in", 512)], dict(V=512)),
           Case("sample_eos", "tail", "stride (logits, work)",
                [stride_op("logits", "f32", "in", V), stride_op("work", "f32", "out", V)], dict(V=V)),
           # one batch row, two beams: logits row b * K + k at (b * rows_per_batch + k) * ldl
           Case("beam_step_k2", "tail", "stride (logits: rows_per_batch * ldl)", [stride_op("logits", "f32", "in", V)], dict(V=V, K=2))]
    return out


def _gemm_cases():
    """Stride form with M = 2.  far = the operands whose leading dimension is LD_FAR in that case."""
    out = []
    N = 256
    table = (
        # name, far operands, K, tile (0 = auto), split_k, out dtype, residual dtype (None: no residual), epilogue
        ("gemm_a_far_auto_k64", ("a",), 64, 0, 1, "bf16", None, "plain"),
        ("gemm_c_far_bf16_auto_k256", ("c",), 256, 0, 1, "bf16", None, "plain"),
        ("gemm_c_far_f32_auto_k256", ("c",), 256, 0, 1, "f32", None, "plain"),
        ("gemm_r_far_f32_auto", ("r",), 256, 0, 1, "f32", "f32", "bias_gelu_res"),
        ("gemm_r_far_bf16_auto", ("r",), 256, 0, 1, "bf16", "bf16", "bias_gelu_res"),
        ("gemm_all_far_tile1_k64", ("a", "c", "r"), 64, 1, 1, "f32", "f32", "bias_gelu_res"),
        ("gemm_all_far_tile2_k256", ("a", "c", "r"), 256, 2, 1, "f32", "f32", "bias_gelu_res"),
        ("gemm_all_far_tile3_k256", ("a", "c", "r"), 256, 3, 1, "bf16", "bf16", "bias_gelu_res"),
        ("gemm_all_far_tile3_splitk2", ("a", "c", "r"), 256, 3, 2, "f32", "f32", "plain_res"),
        ("gemm_all_far_skinny_rowmajor", ("a", "c", "r"), 256, 4, 1, "f32", "f32", "plain_res"),
        ("gemm_all_far_skinny_packed", ("a", "c", "r"), 256, 6, 1, "bf16", "bf16", "plain_res"),
        ("gemm_all_far_skinny_packed_swiglu", ("a", "c"), 256, 6, 1, "bf16", None, "swiglu"),
        ("gemm_all_far_decode_tile", ("a", "c", "r"), 256, 5, 1, "f32", "f32", "plain_res"),
        ("gemm_all_far_decode_tile_splitk2", ("a", "c", "r"), 256, 5, 2, "f32", "f32", "plain_res"),
        ("gemm_all_far_fp8w", ("a", "c", "r"), 256, "fp8w", 1, "f32", "f32", "plain_res"),
        ("gemm_all_far_splitk4_auto", ("a", "c", "r"), 512, 0, 4, "f32", "f32", "plain_res"),
        ("gemm_all_far_splitk4_bias_gelu", ("a", "c", "r"), 512, 2, 4, "bf16", "bf16", "bias_gelu_res"),
        ("gemm_swiglu_far_auto", ("a", "c"), 256, 0, 1, "bf16", None, "swiglu"),
        ("gemm_inplace_residual_far", ("a", "c"), 256, 0, 1, "f32", "inplace", "plain_res"),
        ("gemm_ldw_2rows", ("a", "c"), 64, 0, 1, "f32", None, "plain_w"),          # W: 2 rows, ldw = LD_FAR (below)
    )
    for name, far, K, tile, split_k, out_dt, res_dt, epi in table:
        n_w = 2 if epi == "plain_w" else N
        n_out = n_w // 2 if epi == "swiglu" else n_w

        def mk(nm, dt, role, n):
            return stride_op(nm, dt, role, n) if nm in far else plain_op(nm, dt, role, n, 2)
        inplace = res_dt == "inplace"
        ops = [mk("a", "bf16", "in", K), mk("c", out_dt, "inout" if inplace else "out", n_out)]
        if res_dt and not inplace:
            ops.append(mk("r", res_dt, "in", n_out))
        if epi == "plain_w":        # the weight itself in stride form: two rows is what fits the arena at ldw = LD_FAR (a uniform
            ops.append(stride_op("w", "bf16", "in", K))   # row stride with more rows would put some in [2^31, 2^32) below the pointer)
        out.append(Case(name, "gemm", "stride", ops, dict(N=n_w, K=K, tile=tile, split_k=split_k, epi=epi, inplace=inplace)))
    # gemm_rmsnorm: C, residual and xn far; split_k 1 (the GEMM's own epilogue, then icl_rmsnorm since ldc != N) and 4 (the fused
    # slab reduce + RMSNorm kernel, whose coff / roff are the far ones)
    for name, tile, split_k, K in (("gemm_rmsnorm_far", 0, 1, 256), ("gemm_rmsnorm_far_splitk4", 0, 4, 512),
                                   ("gemm_rmsnorm_far_skinny", 4, 1, 256)):
        ops = [stride_op("a", "bf16", "in", K), stride_op("c", "f32", "out", N), stride_op("r", "f32", "in", N),
               stride_op("xn", "bf16", "out", N)]
        out.append(Case(name, "gemm_rmsnorm", "stride", ops, dict(N=N, K=K, tile=tile, split_k=split_k)))
    # batched form: batch = 2 with stride_a / stride_c / stride_r = LD_FAR.  M = 256 rows per batch (contiguous, ld = row length), so
    # that the tiles are INTERIOR ones: with M = 2 above only the bounds-checked edge paths run, and the interior epilogues (the
    # vector stores of tiles 1 / 2, the LDS-staged whole-row stores and the whole-row residual loads of tile 3) carry address
    # arithmetic of their own.  A "row" of these operands is one batch's whole matrix.
    Mb, K = 256, 128
    for name, tile, out_dt, res_dt, epi in (("gemm_batched_tile1_f32", 1, "f32", "f32", "bias_gelu_res"),
                                            ("gemm_batched_tile2_bf16", 2, "bf16", "bf16", "bias_gelu_res"),
                                            ("gemm_batched_tile3_f32_res", 3, "f32", "f32", "bias_res"),
                                            ("gemm_batched_tile3_bf16", 3, "bf16", None, "bias"),
                                            ("gemm_batched_tile3_swiglu", 3, "bf16", None, "swiglu"),
                                            ("gemm_batched_auto_f32", 0, "f32", "bf16", "bias_res")):
        n_out = N // 2 if epi == "swiglu" else N

        def bop(nm, dt, role, ld):
            return Op(nm, dt, role, Mb * ld, (0, LD_FAR), (0, compact_ld(Mb * ld)),
                      meta=dict(ld=ld, ld_twin=ld, stride=LD_FAR, stride_twin=compact_ld(Mb * ld)))
        ops = [bop("a", "bf16", "in", K), bop("c", out_dt, "out", n_out)]
        if res_dt:
            ops.append(bop("r", res_dt, "in", n_out))
        out.append(Case(name, "gemm_batched", "stride (batch)", ops, dict(N=N, K=K, M=Mb, tile=tile, epi=epi)))
    return out


GRID_LENS_LAST = (1, 65, 320)           # lengths of the last three sequences (the issue's); every unchecked sequence has 1
GRID_ROWS = 320                         # positions of a checked sequence that hold data
# (elements per sequence, sequences): 1030 x 2^22 (1 head x 32 768 positions x 128) is more than 1024 (sequence, head) pairs, the
# many-sequence instantiation of the decode kernels; 260 x 2^24 is the few-sequence one.  The last three start beyond 2^32.
GRID_MANY, GRID_FEW = (1 << 22, 1030), (1 << 24, 260)


def grid_checked(geom):
    """The sequences whose rows are filled and compared: the first three, one whose offset lies in [2^31, 2^32) (a negative
    int32), the last three.  -> {sequence: length}"""
    seq_elems, nseq = geom
    mid = (3 << 30) // seq_elems                # element offset 3 * 2^30
    return {0: 3, 1: 33, 2: 64, mid: 1, nseq - 3: GRID_LENS_LAST[0], nseq - 2: GRID_LENS_LAST[1], nseq - 1: GRID_LENS_LAST[2]}


def _grid_ops(D, geom, dtype="bf16", names=("kc", "vc")):
    """Caches [n_seqs][1 head][max_len][D] walked by block id.  Only the first GRID_ROWS positions of the checked sequences are
    rows (and windows); the twin has the same number of sequences at max_len = GRID_ROWS."""
    seq_elems, nseq = geom
    checked = tuple(grid_checked(geom))
    n = GRID_ROWS * D
    offs, twin = tuple(s * seq_elems for s in checked), tuple(s * n for s in checked)
    meta = dict(max_len=seq_elems // D, max_len_twin=GRID_ROWS, seq_elems=seq_elems, nseq=nseq)
    return [Op(nm, dtype, "in", n, offs, twin, low=(1 << 31) * ESIZE[dtype], meta=dict(meta)) for nm in names]


def _decode_cases():
    out = []
    for name, D, geom in (("attn_decode_d128_many", 128, GRID_MANY), ("attn_decode_d64_many", 64, GRID_MANY),
                          ("attn_decode_d128_few", 128, GRID_FEW), ("attn_decode_d64_few", 64, GRID_FEW),
                          ("attn_decode_bf16_epl16_d128_many", 128, GRID_MANY), ("attn_decode_bf16_epl16_d64_few", 64, GRID_FEW)):
        out.append(Case(name, "decode", "grid-walk (cache)", _grid_ops(D, geom), dict(D=D, H=1, geom=geom)))
    return out


def _decode_more_cases():
    out = []
    # grouped-query attention: one K/V head serves four query heads; more than 1024 (sequence, K/V head) pairs
    out.append(Case("attn_decode_gqa_g4_many", "decode_gqa", "grid-walk (cache)", _grid_ops(128, GRID_MANY),
                    dict(D=128, H=4, Hkv=1, geom=GRID_MANY)))
    # fp8 cache: the byte planes in grid-walk form (a uint8 element is a byte: sequences of 2^22 bytes), the f32 scale planes
    # [n_seqs][1][max_len] beside them (near: a plane is 4 / D of its byte plane)
    for name, D, geom in (("attn_decode_fp8_d128_many", 128, GRID_MANY), ("attn_decode_fp8_d64_few", 64, GRID_FEW)):
        ops = _grid_ops(D, geom, "u8", ("kc", "vc"))
        seq_elems, nseq = geom
        checked = tuple(grid_checked(geom))
        for nm in ("ks", "vs"):
            ops.append(Op(nm, "f32", "in", GRID_ROWS, tuple(s * (seq_elems // D) for s in checked), tuple(s * GRID_ROWS for s in checked)))
        out.append(Case(name, "decode_fp8", "grid-walk (byte planes)", ops, dict(D=D, H=1, geom=geom)))
    return out


FUSED_MAXLEN = 64


def _fused_cases():
    """attn_decode_rope: qkv rows far (stride form), cache rows far (index form through seq_ids).  Two sequences, lengths
    ROPE_POS + 1; a row of the cache operands is one (sequence, head) stripe of max_len positions, of which the launch reads the
    first len - 1 and writes position len - 1."""
    H, D = ROPE_H, 128
    seq_elems = H * FUSED_MAXLEN * D

    def rows(ids):
        return tuple(s * seq_elems + h * FUSED_MAXLEN * D for s in ids for h in range(H))
    twin_ids = (0, 1)
    ops = [stride_op("qkv", "bf16", "in", 3 * H * D), stride_op("out", "bf16", "out", H * D)]
    for nm in ("kc", "vc"):
        ops.append(Op(nm, "bf16", "inout", FUSED_MAXLEN * D, rows(ROPE_SIDS), rows(twin_ids), meta=dict(ids=ROPE_SIDS, ids_twin=twin_ids)))
    cases = [Case("attn_decode_rope", "decode_rope", "stride (qkv, out) + index (cache)", ops, dict(H=H, D=D, fp8=False))]
    # the fp8 form: byte planes in the same places (a byte per element), the f32 scale planes [n_seqs][H][max_len] beside them
    ops = [stride_op("qkv", "bf16", "in", 3 * H * D), stride_op("out", "bf16", "out", H * D)]
    for nm in ("kc", "vc"):
        ops.append(Op(nm, "u8", "inout", FUSED_MAXLEN * D, rows(ROPE_SIDS), rows(twin_ids), meta=dict(ids=ROPE_SIDS, ids_twin=twin_ids)))

    def srows(ids):
        return tuple((s * H + h) * FUSED_MAXLEN for s in ids for h in range(H))
    for nm in ("ks", "vs"):
        ops.append(Op(nm, "f32", "inout", FUSED_MAXLEN, srows(ROPE_SIDS), srows(twin_ids)))
    cases.append(Case("attn_decode_rope_fp8", "decode_rope", "stride (qkv, out) + index (byte planes)", ops, dict(H=H, D=D, fp8=True)))
    return cases


COPY_H, COPY_T, COPY_D, COPY_N = 2, 64, 128, 6        # heads, positions, head_dim of the copied caches; positions per span


def _copy_cases():
    """kv_copy_spans: spans (src_seq, src_t0) -> (dst_seq, dst_t0) for every layer and head.  far_seq: one layer, sequence ids
    beyond 2^32 elements on both sides; far_layer: two layers whose stride is LD_FAR (the beam search's l * s_layer)."""
    out = []
    s_seq = COPY_H * COPY_T * COPY_D
    spans = dict(src_seq=(262147, 1), src_t0=(3, 9), dst_seq=(2, 262146), dst_t0=(0, 20))
    for fp8 in (False, True):
        dt = "u8" if fp8 else "bf16"
        for name, L, far_ids in (("far_seq", 1, True), ("far_layer", 2, False)):
            ops = []
            for side, role in (("src", "in"), ("dst", "out")):
                ids = spans[side + "_seq"] if far_ids else (2, 0)
                t0 = spans[side + "_t0"]
                twin_ids = tuple(sorted(ids).index(i) * 2 + 1 for i in ids)            # distinct small ids, not 0, 1, ..
                n_seqs, n_twin = max(ids) + 1, max(twin_ids) + 1
                s_layer, s_layer_twin = (LD_FAR, n_twin * s_seq + 64) if L > 1 else (0, 0)      # + 64: LD_FAR's residue mod 128

                def offs(id_list, layer_stride, per_pos):
                    # per_pos = elements per position: D for the rows, 1 for a scale plane
                    return tuple(l * layer_stride + s * (COPY_H * COPY_T * per_pos) + h * (COPY_T * per_pos) + t * per_pos
                                 for l in range(L) for s, t in zip(id_list, t0) for h in range(COPY_H))
                meta = dict(ids=ids, ids_twin=twin_ids, n_seqs=n_seqs, n_seqs_twin=n_twin, s_layer=s_layer, s_layer_twin=s_layer_twin)
                ops.append(Op(side, dt, role, COPY_N * COPY_D, offs(ids, s_layer, COPY_D), offs(twin_ids, s_layer_twin, COPY_D),
                              meta=dict(meta)))
                if fp8:      # the scale planes [L][n_seqs][H][T] f32 (near: 4 / D of the byte plane); their layer stride is compact
                    pl, pl_twin = n_seqs * COPY_H * COPY_T, n_twin * COPY_H * COPY_T
                    ops.append(Op(side + "_scale", "f32", role, COPY_N, offs(ids, pl, 1), offs(twin_ids, pl_twin, 1),
                                  meta=dict(meta, s_layer=pl, s_layer_twin=pl_twin)))
            out.append(Case(f"kv_copy_spans_{'fp8' if fp8 else 'bf16'}_{name}", "kv_copy", "index (sequence ids)" if far_ids else
                            "stride (layer)", ops, dict(L=L, fp8=fp8, t0=dict(src=spans["src_t0"], dst=spans["dst_t0"]))))
    return out


QF_WIN, QF_RPA = 8, (1 << 25) + 8           # rows per audio: audio 1 starts at row 2^25 + 8 = element 2^32 + 1024 of kv (ldkv = 128)


def _qformer_cases():
    ldkv = 128                               # one head: K at column 0, V at column 64
    kv = Op("kv", "bf16", "in", QF_WIN * ldkv, (0, QF_RPA * ldkv), (0, QF_WIN * ldkv), meta=dict(rpa=QF_RPA, rpa_twin=QF_WIN, ld=ldkv,
                                                                                                 ld_twin=ldkv))
    return [Case("qformer_window_xattn", "qformer", "stride (q, out) + rows_per_audio (kv)",
                 [stride_op("q", "bf16", "in", 64), kv, stride_op("out", "bf16", "out", 64)], dict(H=1, win=QF_WIN))]


def _prefill_cases():
    """attn_fwd.  Packed rows with far ldq / ldk / ldv / ldo (stride form, two sequences of length 1): D = 64 non-causal (the
    interleaved kernel), D = 128 causal, and the suffix-query form.  The cache layout in grid-walk form (kv_seq_stride = 2^22 from
    the binding's n_kv_heads * max_len * head_dim), D = 128 causal and D = 64 non-causal with one head, and a grouped-query case
    (two query heads on one K/V head)."""
    out = []
    for name, D, causal, suffix in (("attn_fwd_packed_d64", 64, False, False), ("attn_fwd_packed_d128_causal", 128, True, False),
                                    ("attn_fwd_suffix_d128", 128, True, True)):
        H = 2
        ops = [stride_op(nm, "bf16", "in", H * D) for nm in ("q", "k", "v")] + [stride_op("out", "bf16", "out", H * D)]
        out.append(Case(name, "prefill", "stride (ldq, ldk, ldv, ldo)", ops, dict(H=H, D=D, causal=causal, suffix=suffix)))
    return out


def _prefill_cache_cases():
    out = []
    for name, D, H, causal in (("attn_fwd_cache_d128_causal", 128, 1, True), ("attn_fwd_cache_d64", 64, 1, False),
                               ("attn_fwd_cache_gqa_d128_causal", 128, 2, True)):
        out.append(Case(name, "prefill_cache", "grid-walk (cache layout)", _grid_ops(D, GRID_MANY),
                        dict(D=D, H=H, Hkv=1, causal=causal, geom=GRID_MANY)))
    return out


def _fused_gemm_cases():
    """icl_gemm_rope_kv_bf16 (the 256x256 tile's fused RoPE + append epilogue): A and C rows far (stride form), cache rows far (index
    form through seq_ids); the shapes of the rope_kv case."""
    H, D, K, M = ROPE_H, 128, 128, len(ROPE_SIDS)
    seq_elems = H * ROPE_MAXLEN * D

    def rows(ids):
        return tuple(s * seq_elems + h * ROPE_MAXLEN * D + p * D for s, p in zip(ids, ROPE_POS) for h in range(H))
    twin_ids = tuple(range(M))
    ops = [stride_op("a", "bf16", "in", K), stride_op("c", "bf16", "out", 3 * H * D)]
    for nm in ("kc", "vc"):
        ops.append(Op(nm, "bf16", "out", D, rows(ROPE_SIDS), rows(twin_ids), meta=dict(ids=ROPE_SIDS, ids_twin=twin_ids)))
    return [Case("gemm_rope_kv", "gemm_rope", "stride (A, C) + index (cache)", ops, dict(H=H, D=D, K=K, M=M))]


SM_MAXLEN, SM_LENS, SM_NSEG = 64, (6, 64), 3
SM_QROWS = (3, (1 << 25) + 5)               # q_rows: rows of 128 elements, the second beyond 2^32 elements


def _segmass_cases():
    """attn_segmass.  grid: the K cache in grid-walk form (mass is contiguous by contract and stays near).  stride: two sequences
    with seg rows (uint8) at row stride LD_FAR, probs rows at ld_probs = LD_FAR and the queries picked by far q_rows."""
    grid = Case("attn_segmass_grid", "segmass", "grid-walk (Kc)", _grid_ops(128, GRID_MANY, names=("kc",)),
                dict(D=128, H=1, geom=GRID_MANY))
    ops = [index_op("q", "bf16", "in", 128, 128, SM_QROWS), Op("seg", "u8", "in", SM_MAXLEN, (0, LD_FAR), (0, 192), meta=dict(ld=LD_FAR, ld_twin=192)),      # 192: LD_FAR bytes mod 128
           stride_op("probs", "f32", "out", SM_MAXLEN)]
    return [place_grid(grid), place(Case("attn_segmass_stride", "segmass", "stride (seg, ld_probs) + index (q_rows)", ops,
                                         dict(D=128, H=1)))]


def place_grid(case):
    """Grid-walk: the first cache at the first SLOT multiple that leaves 2^31 elements (and a margin) below it; every further
    operand a SLOT plus a fraction of a sequence stripe above the one before, so that sequence b of one never meets a row of
    another (a stripe is at least 4 MiB, a checked sequence's rows at most 80 KiB)."""
    base = (max(o.low for o in case.ops) + MARGIN + SLOT - 1) // SLOT * SLOT
    for i, o in enumerate(case.ops):
        o.base = base + i * (SLOT + (1 << 20) + (3 << 16))        # + 192 KiB: an fp8 scale plane's sequences are 128 KiB or 1 MiB apart
    return case


def all_cases():
    cases = _norm_cases() + _rope_cases() + _glue_cases() + _tail_cases() + _gemm_cases() + _fused_cases() + _copy_cases() + _qformer_cases() + _prefill_cases() + _fused_gemm_cases()
    cases = [place(c) for c in cases] + [place_grid(c) for c in _decode_cases() + _decode_more_cases() + _prefill_cache_cases()]
    cases += _segmass_cases()
    # the audio front end: two clips at wav_ld = LD_FAR (the entry point refuses an xt_ld above 128, so the log-mel output's xt
    # cannot be far; the GPU module asserts that refusal)
    cases += [place(Case("logmel_whisper", "frontend", "stride (wav_ld)", [stride_op("wav", "f32", "in", 8000)], dict(lens=(8000, 150)))),
              place(Case("fbank_kaldi", "frontend", "stride (wav_ld)", [stride_op("wav", "f32", "in", 2960)], dict(lens=(2960, 560))))]
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = all_cases()
BY_NAME = {c.name: c for c in CASES}


def group(name):
    return [c for c in CASES if c.group == name]


# ------------------------------------------------------------------------------------------------------------------
# the CPU model of a launch, and the GPU test's verdict on it
# ------------------------------------------------------------------------------------------------------------------
class SparseMem:
    """One operand's memory as a dict of windows (float64 values, one per element): sentinel everywhere, data in the input rows,
    NaN in the output rows — what the GPU test's setup writes."""
    SENT = -77.0

    def __init__(self, op, offs, seed):
        self.op, self.offs, es = op, offs, op.esize
        self.win = {}
        for lo, hi in op.windows(offs, margin=1024):          # the model needs the windows' places, not their full margins
            assert lo % es == 0 and hi % es == 0
            self.win[lo // es] = np.full((hi - lo) // es, self.SENT)
        rng = np.random.default_rng(seed)
        for i, o in enumerate(offs):
            self.write(o, rng.normal(size=op.n) if op.role != "out" else np.full(op.n, np.nan))
        self.before = {k: v.copy() for k, v in self.win.items()}

    def _find(self, e, n):
        for lo, arr in self.win.items():
            if lo <= e and e + n <= lo + len(arr):
                return arr, e - lo
        raise IndexError(f"{self.op.name}: elements [{e}, {e + n}) are outside every compared window")

    def read(self, e):
        arr, i = self._find(e, self.op.n)
        return arr[i:i + self.op.n].copy()

    def write(self, e, vals):
        arr, i = self._find(e, self.op.n)
        arr[i:i + self.op.n] = vals

    def unexpected_change(self):
        """True when an element outside the expected output rows differs from its pre-launch value (assertion 3)."""
        for lo, arr in self.win.items():
            keep = np.ones(len(arr), bool)
            for o in (self.offs if self.op.role != "in" else ()):
                a, b = max(o - lo, 0), min(o + self.op.n - lo, len(arr))
                if a < b:
                    keep[a:b] = False
            if not np.array_equal(arr[keep], self.before[lo][keep], equal_nan=True):
                return True
        return False


def emulate(case, far=True, narrowed=None, kind=None):
    """Run the model on the far (or twin) layout with operand `narrowed` addressed through narrowing `kind`.  Returns the
    memories and the output rows read back at their TRUE places, as the GPU test reads them."""
    mems = {o.name: SparseMem(o, o.offs if far else o.twin, seed=zlib.crc32(f"{case.name}/{o.name}".encode())) for o in case.ops}

    def addr(o, off):
        return narrow(off, o.esize, kind) // o.esize if (o.name == narrowed and far) else off
    n_rows = max(len(o.offs) for o in case.ops)
    aux = {}
    for i in range(n_rows):
        acc = 1.0
        for o in case.ops:
            if o.role != "out":
                offs = mems[o.name].offs
                acc = acc + mems[o.name].read(addr(o, offs[i % len(offs)])).sum()
        for o in case.ops:
            if o.role != "in":
                offs = mems[o.name].offs
                if i < len(offs):
                    mems[o.name].write(addr(o, offs[i]), np.full(o.n, acc))
        aux[("aux", i)] = np.array([acc])          # what a launch returns in small tensors of its own (token ids, losses, ...)
    outs = {(o.name, i): mems[o.name].read(off) for o in case.ops if o.role != "in" for i, off in enumerate(mems[o.name].offs)}
    outs.update(aux)
    return mems, outs


def verdict(case, narrowed=None, kind=None):
    """Which of the GPU test's assertions fail for the emulated launch: a subset of {1, 3} (2 judges the twin alone)."""
    mems, outs = emulate(case, True, narrowed, kind)
    _, twin = emulate(case, False)
    failed = set()
    if any(not np.array_equal(outs[k], twin[k]) for k in twin):          # NaN != NaN: an unwritten output row fails
        failed.add(1)
    if any(m.unexpected_change() for m in mems.values()):
        failed.add(3)
    return failed

"""`-m gpu`: the segment-to-segment attention flow.  icl_attn_segflow_bf16 against the float64 reference of
tests/attn_segflow_ref.py, per element (the bound and its derivation are in that module's docstring; tests/test_attn_segflow_ref.py
shows on the CPU that it admits an f32 emulation in the kernel's order and rejects every mutant on the cases used here).

Every launch covers sequences of 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200 and 385 positions — every boundary of the 32-query
block, the 128-query workgroup pass and the 64-key tile — at max_len 448, NaN in the cache rows and 0xFF in the segment bytes past
each length, Q a column slice of a wider buffer and flow starting as NaN.  Forms (D, H, Hkv): (64, 3, 3) attn_segflow_kernel<64>;
(128, 4, 4), (128, 4, 2), (128, 8, 1) attn_segflow_kernel<128> at G = 1, 2, 8; n_seg 1, 2 and 32.

Checks: random data against the bound; the count probe (all keys equal: p(i, j) = 1 / (i + 1), flow an exact rational, a query
segment's masses plus the ignored keys' share sum to its rows); the peak probe (a +-1 key pattern picked by every query row); pairs
with nothing to count exactly 0.0; a sequence's bits alone, in the 13-sequence launch, in the reversed batch and among more than
1024 workgroups; Q addressed beyond 2^32 elements against its compact twin; every refusal of the entry point.

Measured on MI355X (printed by the tests, recorded in README.md): largest err / bound over n_seg 1, 2, 32 — random data 0.055 (head_dim
64), 0.024 (128, all three forms); count probe 0.001; peak probe 0.257 (64), 0.354 (128): its far keys, held to the absolute term;
single keys and rows 0.024.
"""
import math

import pytest
import torch

import attn_segflow_ref as fr
import far_layout as fl
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NAN = float("nan")
I32 = torch.int32


def _launch(B, q, kc, lens, seg, n_seg, H, Hkv, D):
    """One launch on device copies; flow starts as NaN, Q is a column slice of a wider buffer.  Returns flow on the CPU."""
    n = len(lens)
    qbuf = torch.full((q.shape[0], H * D + 64), NAN, dtype=torch.bfloat16, device=DEV)
    qbuf[:, 32:32 + H * D] = q.to(DEV)
    flow = torch.full((n, H, n_seg, n_seg), NAN, device=DEV)
    B.attn_segflow(qbuf[:, 32:32 + H * D], torch.tensor(fr.cu_of(lens), dtype=I32, device=DEV), kc.to(DEV), seg.to(DEV), flow, H, D,
                   kc.shape[2], max(lens), D ** -0.5, n_kv_heads=Hkv)
    torch.cuda.synchronize()
    return flow.cpu()


def _assert_bound(flow, R, D, what):
    r = fr.flow_ratio(flow, R, D)
    print(f"err/bound {what}: {float(r.max()):.3f}")
    assert float(r.max()) <= 1, f"{what}: err/bound {float(r.max()):.3g} at {fr.describe(r)}"
    empty = (R.N_ac == 0)[:, None].expand_as(flow)
    assert bool(empty.any()) or flow.shape[-1] == 1
    assert bool((flow[empty] == 0).all()), f"{what}: a pair with nothing to count is not exactly 0.0"
    return float(r.max())


@pytest.mark.parametrize("case", fr.CASES, ids=fr.case_id)
def test_kernel(B, case):
    D, H, Hkv, n_seg = case
    lens, scale = list(fr.LENS), D ** -0.5
    seg = fr.make_seg(lens, n_seg)
    name = f"attn_segflow {fr.case_id(case)}"

    # random data against the bound; two launches give equal bits
    q, kc = fr.random_case(lens, H, Hkv, D)
    R = fr.reference(q, kc, lens, seg, n_seg, H, Hkv, D, scale)
    flow = _launch(B, q, kc, lens, seg, n_seg, H, Hkv, D)
    _assert_bound(flow, R, D, f"{name} normal")
    assert torch.equal(_launch(B, q, kc, lens, seg, n_seg, H, Hkv, D), flow), f"{name}: not reproducible"

    # count probe: p(i, j) = 1 / (i + 1); flow is an exact rational and a query segment's masses plus the ignored share are its rows
    q, kc = fr.count_probe(lens, H, Hkv, D)
    R = fr.reference(q, kc, lens, seg, n_seg, H, Hkv, D, scale)
    want, ign = fr.count_flow(lens, seg, n_seg)
    assert float((R.flow - want[:, None]).abs().max()) < 1e-11
    flow = _launch(B, q, kc, lens, seg, n_seg, H, Hkv, D)
    _assert_bound(flow, R, D, f"{name} count probe")
    rows = R.rows.double()
    total_rel = fr.C1 * D * fr.U * R.S + fr.C2 * (3 * R.n[:, None] + 8) * fr.U + fr.SPLIT            # n_c, n_a <= n in every term of the sum
    total = flow.double().sum(-1) + ign[:, None]
    assert bool(((total - rows[:, None]).abs() <= rows[:, None] * total_rel[:, :, None] + 2 * R.n[:, None, None] ** 2 * fr.TINY).all()), \
        f"{name} count probe: a query segment's masses and its ignored share do not sum to its rows"

    # peak probe: every row's target key holds the row's mass on the reference; the kernel is held to the bound on it
    q, kc = fr.peak_probe(lens, H, Hkv, D, seg, n_seg)
    R = fr.reference(q, kc, lens, seg, n_seg, H, Hkv, D, scale)
    assert R.pmax_min >= fr.W_EXACT
    flow = _launch(B, q, kc, lens, seg, n_seg, H, Hkv, D)
    _assert_bound(flow, R, D, f"{name} peak probe")


@pytest.mark.parametrize("D,H,Hkv", [(128, 4, 4), (64, 3, 3), (128, 8, 1)], ids=["D128", "D64", "gqa8"])
def test_determinism(B, D, H, Hkv):
    """A sequence has the same bits alone, in the 13-sequence launch, in the reversed batch and among more than 1024 workgroups."""
    lens, n_seg = list(fr.LENS), 32
    seg = fr.make_seg(lens, n_seg)
    q, kc = fr.random_case(lens, H, Hkv, D)
    cu = fr.cu_of(lens)
    flow = _launch(B, q, kc, lens, seg, n_seg, H, Hkv, D)
    for b, L in enumerate(lens):
        one = _launch(B, q[cu[b]:cu[b + 1]], kc[b:b + 1], [L], seg[b:b + 1], n_seg, H, Hkv, D)
        assert torch.equal(one[0], flow[b]), f"sequence {b} (len {L}) alone != in the batch"
    rev = list(range(len(lens)))[::-1]
    q_rev = torch.cat([q[cu[b]:cu[b + 1]] for b in rev])
    f_rev = _launch(B, q_rev, kc[rev], [lens[b] for b in rev], seg[rev], n_seg, H, Hkv, D)
    assert torch.equal(f_rev, flow[rev]), "the reversed batch gives other bits"
    reps = 1024 // (len(lens) * H) + 1
    assert len(lens) * reps * H > 1024
    big = _launch(B, q.repeat(reps, 1), kc.repeat(reps, 1, 1, 1), lens * reps, seg.repeat(reps, 1), n_seg, H, Hkv, D)
    assert torch.equal(big, flow.repeat(reps, 1, 1, 1)), "more than 1024 workgroups give other bits"


def test_single_keys_and_rows(B):
    """Segments that hold single keys and single rows: flow[a, c] is the single weight p(a, c), held to the bound (a P rounded once
    to bf16 misses it: tests/test_attn_segflow_ref.py)."""
    D, H = 128, 2
    q, kc, seg = fr.single_case(D, H)
    R = fr.reference(q, kc, [32], seg, 32, H, H, D, D ** -0.5)
    flow = _launch(B, q, kc, [32], seg, 32, H, H, D)
    _assert_bound(flow, R, D, "attn_segflow single keys and rows")


# ------------------------------------------------------------------------------------------------------------------
# far offsets: Q rows beyond 2^32 elements
# ------------------------------------------------------------------------------------------------------------------
def test_far_q_offset(B):
    """Two sequences of one position each, Q at ldq = 2^32 + 64 over the 16.25 GiB arena of tests/far_layout.py: packed row 1 (the
    second sequence's only query) starts beyond 2^32 elements.  (1) flow equals the compact twin's bit for bit, (2) the twin is
    inside the bound, (3) the arena around the rows is untouched (Q is an input; flow lives in a tensor of its own).  A leading
    dimension narrowed to 32 bits is 64: it would read row 0's sentinel-filled neighbourhood."""
    need = fl.ARENA_BYTES + (4 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"free device memory {free} B is below the arena + 4 GiB = {need} B")
    D, H, n_seg, lens = 128, 2, 2, [1, 1]
    op = fl.place(fl.Case("attn_segflow_q", "segflow", "stride (ldq)", [fl.stride_op("q", "bf16", "in", H * D)])).op("q")
    q, kc = fr.random_case(lens, H, H, D, max_len=64)
    seg = torch.full((2, 64), 0xFF, dtype=torch.uint8)
    seg[0, 0], seg[1, 0] = 1, 0
    cu = torch.tensor([0, 1, 2], dtype=I32, device=DEV)
    res = []
    arena = torch.empty(fl.ARENA_BYTES, dtype=torch.uint8, device=DEV)
    try:
        for far in (True, False):
            offs, ld = (op.offs, op.meta["ld"]) if far else (op.twin, op.meta["ld_twin"])
            wins = op.windows(offs)
            for lo, hi in wins:
                arena[op.base + lo:op.base + hi].fill_(fl.SENTINEL)
            view = arena[op.base:op.base + (offs[1] + H * D) * 2].view(torch.bfloat16).as_strided((2, H * D), (ld, 1))
            view.copy_(q.to(DEV))
            before = [arena[op.base + lo:op.base + hi].clone() for lo, hi in wins]
            flow = torch.full((2, H, n_seg, n_seg), NAN, device=DEV)
            B.attn_segflow(view, cu, kc.to(DEV), seg.to(DEV), flow, H, D, 64, 1, D ** -0.5)
            torch.cuda.synchronize()
            assert all(torch.equal(arena[op.base + lo:op.base + hi], bf) for (lo, hi), bf in zip(wins, before)), "(3) the arena changed"
            res.append(flow.cpu())
    finally:
        del arena
        torch.cuda.empty_cache()
    assert torch.equal(res[0], res[1]), "(1) the far launch differs from the twin"
    R = fr.reference(q, kc, lens, seg, n_seg, H, H, D, D ** -0.5)
    _assert_bound(res[1], R, D, "attn_segflow far twin")
    assert float(res[1][0, 0, 1, 1]) == 1.0 and float(res[1][1, 0, 0, 0]) == 1.0


# ------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------
def test_entry_point_refusals(B):
    """Every -1 refusal of the entry point, on device operands, naming the argument; then the binding raises on the same."""
    lib = B.load_library()
    D, H, lens = 128, 4, [5, 9]
    q, kc = fr.random_case(lens, H, H, D, max_len=16)
    seg = fr.make_seg(lens, 2, max_len=16)
    _launch(B, q, kc, lens, seg, 2, H, H, D)                                         # the valid call
    qd, kd, sd = q.to(DEV), kc.to(DEV), seg.to(DEV)
    cu = torch.tensor(fr.cu_of(lens), dtype=I32, device=DEV)
    flow = torch.zeros(2, H, 2, 2, device=DEV)
    good = dict(Q=qd.data_ptr(), ldq=H * D, cu=cu.data_ptr(), Kc=kd.data_ptr(), seg=sd.data_ptr(), ld_seg=16, n_seg=2,
                flow=flow.data_ptr(), n_seqs=2, n_heads=H, n_kv_heads=0, head_dim=D, max_len=16, max_seqlen=9, scale=D ** -0.5,
                stream=None)

    def refused(word, **kw):
        rc = lib.icl_attn_segflow_bf16(*dict(good, **kw).values())
        msg = lib.icl_last_error()
        assert rc == -1 and b"icl_attn_segflow_bf16" in msg and word in msg, (kw, rc, msg)

    for name in ("Q", "cu", "Kc", "seg", "flow"):
        refused(name.encode(), **{name: None})
    refused(b"n_seg", n_seg=0)
    refused(b"n_seg", n_seg=33)
    refused(b"head_dim", head_dim=96)
    refused(b"n_kv_heads", n_kv_heads=3)
    refused(b"n_kv_heads", n_heads=18, n_kv_heads=2, ldq=18 * 128)                   # G = 9
    refused(b"head_dim", n_kv_heads=2, head_dim=64)                                  # G = 2 at head_dim 64
    refused(b"n_seqs", n_seqs=0)
    refused(b"n_seqs", n_seqs=65536)
    refused(b"max_seqlen", max_seqlen=0)
    refused(b"max_seqlen", max_seqlen=17)
    refused(b"ld_seg", ld_seg=15)
    refused(b"ldq", ldq=H * D + 4)
    refused(b"ldq", ldq=H * D - 8)
    refused(b"Q", Q=qd.data_ptr() + 8)
    refused(b"Kc", Kc=kd.data_ptr() + 8)
    refused(b"flow", flow=flow.data_ptr() + 2)
    for bad in (math.inf, -math.inf, math.nan):
        refused(b"scale", scale=bad)
    assert lib.icl_attn_segflow_bf16(*good.values()) == 0
    torch.cuda.synchronize()
    for kw in (dict(D=96), dict(Hkv=3), dict(scale=float("inf")), dict(seg=sd[:, :15].contiguous()), dict(max_seqlen=17)):
        a = dict(dict(D=D, Hkv=0, scale=D ** -0.5, seg=sd, max_seqlen=9), **kw)
        with pytest.raises(B.IclError, match="icl_attn_segflow_bf16"):
            B.attn_segflow(qd, cu, kd, a["seg"], flow, H, a["D"], 16, a["max_seqlen"], a["scale"], n_kv_heads=a["Hkv"])

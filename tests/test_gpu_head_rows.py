"""`-m gpu`: icl_head_rows_bf16, the capture / patch launch on single heads of listed rows of the bf16 attention output, against the
float64 reference and with the assertions of tests/head_rows_ref.py (tests/test_head_rows_ref.py shows on the CPU that they admit
an f32 emulation of the kernel and reject eight one-mistake mutants).

Every launch of a (head_dim, n_heads, n_rows) shape — (64, 3), (128, 4), (128, 40); 1, 3 or 65 of 70 rows; 1, 2 (unsorted) and all
heads selected — works on att as a column slice (ld_att = n_heads * head_dim + 8) of a buffer filled with a sentinel bit pattern:
capture only, replace and add with and without a capture, per-row and shared vectors.  Capture, unlisted rows, unselected heads,
the pad columns and replace (of bf16-valued vectors full of NaN payloads, -0.0, +-inf and subnormals: their bits; of arbitrary f32:
bf16_rne) are compared as bits; add is held to bf16_interval(ref, 2^-24 |ref| + 2^-149) on normal data, data scaled by 2^-20 and
2^20 and the cancellation probe.  Then: a list and its reverse give the same bits; one far-offset launch (ld_att = 2^32 + 64 over the
16.25 GiB arena of tests/far_layout.py, rows 0 and 1) against a compact twin, bit for bit; the refusals of the entry point, through
the raw call and through the binding.

Measured on MI355X: see README.md, "Attention-head output capture and patching".
"""
import numpy as np
import pytest
import torch

import far_layout as fl
import head_rows_ref as hr
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

F32, BF16, I32, I16, U8 = torch.float32, torch.bfloat16, torch.int32, torch.int16, torch.uint8


def _bits(a: np.ndarray) -> torch.Tensor:
    """uint16 bits -> a bf16 tensor on the device."""
    return torch.from_numpy(a.view(np.int16).copy()).to(DEV).view(BF16)


def _np(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(I16).cpu().numpy().view(np.uint16)


def _launch(B, c, att, rows, heads, vec):
    """One launch of case ``c`` on the numpy inputs -> (att_out uint16 [70, ld], cap uint16 [n, width] | None)."""
    full = _bits(att)
    av = full[:, :c.width]                                   # the column slice: ld_att = width + PAD
    cap = _bits(np.full((c.n_rows, c.width), hr.SENTINEL, dtype=np.uint16)) if c.capture else None
    v = None if vec is None else torch.from_numpy(vec.copy()).to(DEV)
    h = None if heads is None else torch.from_numpy(heads.copy()).to(DEV)
    B.head_rows(av, torch.from_numpy(rows.copy()).to(DEV), n_heads=c.H, head_dim=c.D, capture=cap, heads=h, vec=v,
                mode=c.mode or "replace", alpha=c.alpha)
    torch.cuda.synchronize()
    return _np(full), (None if cap is None else _np(cap))


@pytest.mark.parametrize("n_rows", hr.N_ROWS)
@pytest.mark.parametrize("D,H", hr.SHAPES)
def test_every_launch_of_a_shape(B, D, H, n_rows):
    worst = 0.0
    for c in hr.launch_cases(D, H, n_rows):
        args = hr.inputs(c)
        out, cap = _launch(B, c, *args)
        fails, w = hr.check(c, hr.expect(c, *args), out, cap)
        assert not fails, (c.id, fails)
        worst = max(worst, w)
    print(f"head_rows D {D} H {H} n_rows {n_rows}: add, largest interval_ratio {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("mode", ["replace", "add"])
def test_a_list_and_its_reverse_give_the_same_bits(B, mode):
    base = hr.Launch(128, 4, 65, "two", True, mode, False, "bits" if mode == "replace" else "normal", 0.7)
    (a0, r0, h0, v0), (a1, r1, h1, v1) = (hr.inputs(c) for c in (base, hr.Launch(**{**base.__dict__, "reverse": True})))
    assert np.array_equal(r0, r1[::-1]) and np.array_equal(a0, a1)
    o0, c0 = _launch(B, base, a0, r0, h0, v0)
    o1, c1 = _launch(B, base, a1, r1, h1, v1)
    assert np.array_equal(o0, o1) and np.array_equal(c0, c1[::-1])
    assert not np.array_equal(o0, a0)


# ------------------------------------------------------------------------------------------------------------------
# far offsets: ld_att = 2^32 + 64
# ------------------------------------------------------------------------------------------------------------------
class _Mem:
    """The operands of ``hr.far_case()`` as views into the arena (far) or into small buffers of their own (the compact twin):
    every compared window filled with the sentinel byte, then the rows with the same values in both."""

    def __init__(self, case, arena):
        self.case, self.far = case, arena is not None
        self.buf, self.base, self.before = {}, {}, {}
        for o in case.ops:
            offs = o.offs if self.far else o.twin
            wins = o.windows(offs)
            base = o.base if self.far else fl.MARGIN
            buf = arena if self.far else torch.empty(base + wins[-1][1], dtype=U8, device=DEV)
            assert base + wins[0][0] >= 0 and base + wins[-1][1] <= buf.numel()
            self.buf[o.name], self.base[o.name] = buf, base
            for lo, hi in wins:
                buf[base + lo:base + hi].fill_(fl.SENTINEL)
            for i, off in enumerate(offs):
                g = torch.Generator().manual_seed(100 * len(o.name) + i)
                if o.role != "out":
                    self.row(o, off).copy_(torch.randn(o.n, generator=g).to(self.dtype(o)))
            self.before[o.name] = [buf[base + lo:base + hi].cpu() for lo, hi in wins]

    @staticmethod
    def dtype(o):
        return F32 if o.dtype == "f32" else BF16

    def row(self, o, off):
        start = self.base[o.name] + off * o.esize
        return self.buf[o.name][start:start + o.n * o.esize].view(self.dtype(o))

    def rows2d(self, name):
        o = self.case.op(name)
        buf, base = self.buf[name], self.base[name]
        ld = o.meta["ld"] if self.far else o.meta["ld_twin"]
        return buf[base:base + (buf.numel() - base) // o.esize * o.esize].view(self.dtype(o)).as_strided((2, o.n), (ld, 1))

    def finish(self):
        """(the rows of att and capture at their true places as bits, what changed outside them)."""
        torch.cuda.synchronize()
        outs, bad = {}, []
        for o in self.case.ops:
            offs, base, buf = (o.offs if self.far else o.twin), self.base[o.name], self.buf[o.name]
            if o.role != "in":
                for i, off in enumerate(offs):
                    outs[(o.name, i)] = self.row(o, off).view(I16).cpu()
            for (lo, hi), before in zip(o.windows(offs), self.before[o.name]):
                keep = torch.ones(hi - lo, dtype=torch.bool)
                for a, b in o.expected(offs):
                    keep[max(a - lo, 0):max(min(b - lo, hi - lo), 0)] = False
                diff = (buf[base + lo:base + hi].cpu() != before) & keep
                if bool(diff.any()):
                    bad.append(f"{o.name}: {int(diff.sum())} bytes outside the expected outputs changed, first at byte {lo + int(diff.nonzero()[0])}")
        return outs, bad


def test_far_leading_dimension(B):
    """Rows 0 and 1 of att at ld_att = 2^32 + 64 (row 1 starts beyond 2^32 elements), capture + add of all four heads, unsorted:
    (1) att and capture are bit-identical to the compact twin's, (2) the twin is inside the interval of the float64 reference and
    its capture is the pre-patch row, (3) nothing else in any compared window changed — a leading dimension narrowed to 32 bits
    is 64, inside row 0's window (tests/test_head_rows_ref.py)."""
    need = fl.ARENA_BYTES + (4 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"free device memory {free} B is below the arena + 4 GiB = {need} B")
    case = hr.far_case()
    D, H = hr.FAR_D, hr.FAR_H
    arena = torch.empty(fl.ARENA_BYTES, dtype=U8, device=DEV)
    rows = torch.tensor([0, 1], dtype=I32, device=DEV)
    order = [2, 0, 3, 1]
    heads = torch.tensor(order, dtype=I32, device=DEV)
    res, m = [], None
    try:
        for a in (arena, None):
            m = _Mem(case, a)
            a0 = [m.row(case.op("att"), off).float().cpu() for off in (case.op("att").offs if a is not None else case.op("att").twin)]
            v = [m.row(case.op("vec"), off).cpu() for off in case.op("vec").offs]
            B.head_rows(m.rows2d("att"), rows, n_heads=H, head_dim=D, capture=m.rows2d("capture"), heads=heads,
                        vec=m.rows2d("vec").view(2, H, D), mode="add", alpha=0.7)
            res.append((m.finish(), a0, v))
    finally:
        del arena, m
        torch.cuda.empty_cache()
    ((out_f, bad_f), a0_f, _), ((out_t, bad_t), a0_t, v) = res
    for k in out_t:
        assert torch.equal(out_f[k], out_t[k]), f"(1) {k}: the far launch differs from the twin"
    assert not bad_f and not bad_t, f"(3) {bad_f + bad_t}"
    for i in range(2):
        assert torch.equal(a0_f[i], a0_t[i]) and torch.equal(out_t[("capture", i)].view(BF16).float(), a0_t[i]), i
        vv = torch.empty(H, D, dtype=torch.float64)
        vv[order] = v[i].view(H, D).double()                      # vector s belongs to head order[s]
        ref = float(np.float32(0.7)) * vv.reshape(-1) + a0_t[i].double()
        lo, hi = hr.bf16_interval(ref, hr.add_error(ref))
        assert bool(hr.in_interval(out_t[("att", i)].view(BF16), lo, hi).all()), f"(2) row {i}"


# ------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_and_the_binding_refuse(B):
    """Each refusal is ICL_EINVAL (-1) with the argument named, and nothing is written."""
    lib = B.load_library()
    H, D = 3, 64
    ld = H * D + 8
    att = torch.arange(4 * ld, dtype=F32, device=DEV).reshape(4, ld).to(BF16)
    cap = torch.full((2, ld), -1.0, dtype=BF16, device=DEV)
    vec = torch.full((2, 2, D), 5.0, dtype=F32, device=DEV)
    rows = torch.tensor([1, 3], dtype=I32, device=DEV)
    heads = torch.tensor([2, 0], dtype=I32, device=DEV)
    before = [t.clone() for t in (att, cap, vec)]
    st = torch.cuda.current_stream().cuda_stream
    base = dict(att=att.data_ptr(), ld_att=ld, rows=rows.data_ptr(), n_rows=2, n_heads=H, head_dim=D, capture=cap.data_ptr(), ld_cap=ld,
                heads=heads.data_ptr(), n_sel=2, vec=vec.data_ptr(), ld_vec=2 * D, mode=1, alpha=0.5)

    def call(**kw):
        a = dict(base, **kw)
        return lib.icl_head_rows_bf16(a["att"], a["ld_att"], a["rows"], a["n_rows"], a["n_heads"], a["head_dim"], a["capture"],
                                      a["ld_cap"], a["heads"], a["n_sel"], a["vec"], a["ld_vec"], a["mode"], a["alpha"], st)
    refusals = {
        "att is NULL": dict(att=0), "rows is NULL": dict(rows=0), "both NULL": dict(capture=0, vec=0), "heads is NULL": dict(heads=0),
        "n_rows": [dict(n_rows=0), dict(n_rows=65536), dict(n_rows=-1)],
        "head_dim": [dict(head_dim=0), dict(head_dim=32), dict(head_dim=96), dict(head_dim=256)],
        "n_heads": [dict(n_heads=0), dict(n_heads=-3)],
        "n_sel": [dict(n_sel=0), dict(n_sel=H + 1), dict(n_sel=-1)],
        "ld_att": [dict(ld_att=H * D - 8), dict(ld_att=H * D + 4)], "ld_cap": [dict(ld_cap=H * D - 8), dict(ld_cap=H * D + 4)],
        "ld_vec": [dict(ld_vec=D), dict(ld_vec=2 * D + 2)],
        "att is not 16-byte": dict(att=att.data_ptr() + 8), "capture is not 16-byte": dict(capture=cap.data_ptr() + 8),
        "vec is not 16-byte": dict(vec=vec.data_ptr() + 4),
        "mode": [dict(mode=2), dict(mode=-1)], "alpha": [dict(alpha=float("nan")), dict(alpha=float("inf"))],
    }
    for word, kws in refusals.items():
        for kw in (kws if isinstance(kws, list) else [kws]):
            assert call(**kw) == -1, (word, kw)
            msg = lib.icl_last_error().decode()
            assert msg.startswith("icl_head_rows_bf16") and word in msg, (word, msg)
    # the same through the binding: an IclError naming the entry point and the argument
    av, cv = att[:, :H * D], cap[:, :H * D]
    ok = dict(att=av, rows=rows, n_heads=H, head_dim=D, capture=cv, heads=heads, vec=vec, mode="add", alpha=0.5)
    for word, kw in {"n_rows": dict(rows=torch.zeros(65536, dtype=I32, device=DEV), capture=None, vec=vec[0]),
                     "head_dim": dict(head_dim=32, vec=torch.zeros(2, 32, device=DEV)), "n_heads": dict(n_heads=0, capture=None),
                     "n_sel": dict(n_heads=1, capture=None), "mode": dict(mode=2), "alpha": dict(alpha=float("inf")),
                     "both NULL": dict(capture=None, vec=None), "16-byte": dict(att=att[:, 4:4 + H * D])}.items():
        a = dict(ok, **kw)
        with pytest.raises(B.IclError, match="icl_head_rows_bf16.*" + word):
            B.head_rows(a.pop("att"), a.pop("rows"), **a)
    with pytest.raises(B.IclError, match="GPU"):
        B.head_rows(av.cpu(), rows, n_heads=H, head_dim=D, capture=cv)
    torch.cuda.synchronize()
    for t, b in zip((att, cap, vec), before):
        assert torch.equal(t.view(I16) if t.dtype == BF16 else t, b.view(I16) if b.dtype == BF16 else b)
    assert call() == 0                                                            # the valid call, last
    torch.cuda.synchronize()
    a0 = before[0]
    assert torch.equal(cap[:, :H * D], a0[[1, 3], :H * D])
    for s, h in enumerate([2, 0]):
        assert torch.equal(att[1, h * D:(h + 1) * D], (a0[1, h * D:(h + 1) * D].float() + 2.5).to(BF16))
    assert torch.equal(att[:, D:2 * D], a0[:, D:2 * D]) and torch.equal(att[:, H * D:], a0[:, H * D:]) and torch.equal(att[0], a0[0])

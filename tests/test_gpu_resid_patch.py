"""`-m gpu`: icl_resid_rows_f32, the capture / patch launch on listed rows of the f32 residual stream, against the float64 reference
and with the assertions of tests/resid_patch_ref.py (tests/test_resid_patch_ref.py shows on the CPU that they admit an f32 emulation
of the kernel and reject six one-mistake mutants).

Every launch of a (hidden, n_rows) shape — hidden 4 (one lane), 1020 (one short of a 1024-element pass), 1024, 1028 (one lane into
the second pass), 5120; 1, 3 or 65 of 70 rows — works on h as a column slice (ldh = hidden + 8) of a buffer filled with a sentinel
bit pattern: capture only, replace and add with and without a capture, per-row and shared vectors.  Capture and replace are compared
as bits on inputs full of NaN payloads, -0.0, +-inf and subnormals; add within (2^-24 + 2^-50) |ref| + 2^-126 on normal data, data
scaled by 2^-20 and 2^20 and the cancellation probe h = -fl32(alpha v); unlisted rows and the 8 columns beyond hidden keep their
bits.  Then: a list and its reverse give the same bits; one far-offset launch (ldh = 2^32 + 64 over the 16.25 GiB arena of
tests/far_layout.py, rows 0 and 1) against a compact twin, bit for bit; the refusals of the entry point through the binding.

Measured on MI355X: see README.md, "Residual-stream capture and patching".
"""
import numpy as np
import pytest
import torch

import far_layout as fl
import resid_patch_ref as rr
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

F32, I32, U8 = torch.float32, torch.int32, torch.uint8


def _launch(B, c, h, rows, vec):
    """One launch of case ``c`` on the numpy inputs -> (h_out f32 [70, ld], cap f32 [n, hidden] | None) as numpy."""
    full = torch.from_numpy(h.copy()).to(DEV)
    hv = full[:, :c.hidden]                                  # the column slice: ldh = hidden + PAD
    cap = torch.full((c.n_rows, c.hidden), float("nan"), dtype=F32, device=DEV) if c.capture else None
    v = None if vec is None else torch.from_numpy(vec.copy()).to(DEV)
    B.resid_rows(hv, torch.from_numpy(rows.copy()).to(DEV), capture=cap, vec=v, mode=c.mode or "replace", alpha=c.alpha)
    torch.cuda.synchronize()
    return full.cpu().numpy(), (None if cap is None else cap.cpu().numpy())


@pytest.mark.parametrize("n_rows", rr.N_ROWS)
@pytest.mark.parametrize("hidden", rr.HIDDENS)
def test_every_launch_of_a_shape(B, hidden, n_rows):
    worst = 0.0
    for c in rr.launch_cases(hidden, n_rows):
        h, rows, vec = rr.inputs(c)
        out, cap = _launch(B, c, h, rows, vec)
        fails, w = rr.check(c, rr.expect(c, h, rows, vec), out, cap)
        assert not fails, (c.id, fails)
        worst = max(worst, w)
        if c.data == "cancel" and hidden * n_rows >= 16:     # the fused form leaves the product's rounding error, not zero
            assert (out[rows, :hidden] != 0).any(), c.id
    print(f"resid_rows hidden {hidden} n_rows {n_rows}: add, largest |out - ref| / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("mode", ["replace", "add"])
def test_a_list_and_its_reverse_give_the_same_bits(B, mode):
    base = rr.Launch(1028, 65, True, mode, False, "bits" if mode == "replace" else "normal", 0.7)
    (h0, r0, v0), (h1, r1, v1) = (rr.inputs(c) for c in (base, rr.Launch(**{**base.__dict__, "reverse": True})))
    assert np.array_equal(r0, r1[::-1]) and np.array_equal(h0.view(np.uint32), h1.view(np.uint32))
    o0, c0 = _launch(B, base, h0, r0, v0)
    o1, c1 = _launch(B, base, h1, r1, v1)
    assert np.array_equal(o0.view(np.uint32), o1.view(np.uint32)) and np.array_equal(c0.view(np.uint32), c1[::-1].view(np.uint32))
    assert not np.array_equal(o0.view(np.uint32), h0.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------
# far offsets: ldh = 2^32 + 64
# ------------------------------------------------------------------------------------------------------------------
class _Mem:
    """The operands of ``rr.far_case()`` as views into the arena (far) or into small buffers of their own (the compact twin):
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
                self.row(o, off).copy_(torch.randn(o.n, generator=g) if o.role != "out" else torch.full((o.n,), float("nan")))
            self.before[o.name] = [buf[base + lo:base + hi].cpu() for lo, hi in wins]

    def row(self, o, off):
        start = self.base[o.name] + off * 4
        return self.buf[o.name][start:start + o.n * 4].view(F32)

    def rows2d(self, name):
        o = self.case.op(name)
        buf, base = self.buf[name], self.base[name]
        ld = o.meta["ld"] if self.far else o.meta["ld_twin"]
        return buf[base:base + (buf.numel() - base) // 4 * 4].view(F32).as_strided((2, o.n), (ld, 1))

    def finish(self):
        """(the rows of h and capture at their true places, what changed outside them)."""
        torch.cuda.synchronize()
        outs, bad = {}, []
        for o in self.case.ops:
            offs, base, buf = (o.offs if self.far else o.twin), self.base[o.name], self.buf[o.name]
            if o.role != "in":
                for i, off in enumerate(offs):
                    outs[(o.name, i)] = self.row(o, off).cpu()
            for (lo, hi), before in zip(o.windows(offs), self.before[o.name]):
                keep = torch.ones(hi - lo, dtype=torch.bool)
                for a, b in o.expected(offs):
                    keep[max(a - lo, 0):max(min(b - lo, hi - lo), 0)] = False
                diff = (buf[base + lo:base + hi].cpu() != before) & keep
                if bool(diff.any()):
                    bad.append(f"{o.name}: {int(diff.sum())} bytes outside the expected outputs changed, first at byte {lo + int(diff.nonzero()[0])}")
        return outs, bad


def test_far_leading_dimension(B):
    """Rows 0 and 1 of h at ldh = 2^32 + 64 (row 1 starts beyond 16 GiB), capture + add: (1) h and capture are bit-identical to the
    compact twin's, (2) the twin is within the bound of the float64 reference, (3) nothing else in any compared window changed —
    a leading dimension narrowed to 32 bits is 64, inside row 0's window (tests/test_resid_patch_ref.py)."""
    need = fl.ARENA_BYTES + (4 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"free device memory {free} B is below the arena + 4 GiB = {need} B")
    case = rr.far_case()
    arena = torch.empty(fl.ARENA_BYTES, dtype=U8, device=DEV)
    rows = torch.tensor([0, 1], dtype=I32, device=DEV)
    res, m = [], None
    try:
        for a in (arena, None):
            m = _Mem(case, a)
            h0 = [m.row(case.op("h"), off).cpu() for off in (case.op("h").offs if a is not None else case.op("h").twin)]
            v = [m.row(case.op("vec"), off).cpu() for off in case.op("vec").offs]
            B.resid_rows(m.rows2d("h"), rows, capture=m.rows2d("capture"), vec=m.rows2d("vec"), mode="add", alpha=0.7)
            res.append((m.finish(), h0, v))
    finally:
        del arena, m
        torch.cuda.empty_cache()
    ((out_f, bad_f), h0_f, _), ((out_t, bad_t), h0_t, v) = res
    bits = lambda t: t.contiguous().view(torch.int32)
    for k in out_t:
        assert torch.equal(bits(out_f[k]), bits(out_t[k])), f"(1) {k}: the far launch differs from the twin"
    assert not bad_f and not bad_t, f"(3) {bad_f + bad_t}"
    for i in range(2):
        assert torch.equal(bits(h0_f[i]), bits(h0_t[i])) and torch.equal(bits(out_t[("capture", i)]), bits(h0_t[i])), i
        ref = float(np.float32(0.7)) * v[i].double() + h0_t[i].double()
        assert bool(((out_t[("h", i)].double() - ref).abs() <= rr.REL * ref.abs() + rr.ABS).all()), f"(2) row {i}"


# ------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------
def test_binding_refuses_what_the_entry_point_refuses(B):
    """Each refusal is ICL_EINVAL (-1) with the argument named, and nothing is written."""
    lib = B.load_library()
    hidden, ld = 8, 16
    h = torch.arange(4 * ld, dtype=F32, device=DEV).reshape(4, ld)
    cap = torch.full((2, ld), -1.0, dtype=F32, device=DEV)
    vec = torch.full((2, ld), 5.0, dtype=F32, device=DEV)
    rows = torch.tensor([1, 3], dtype=I32, device=DEV)
    before = [t.clone() for t in (h, cap, vec)]
    st = torch.cuda.current_stream().cuda_stream
    base = dict(h=h.data_ptr(), ldh=ld, rows=rows.data_ptr(), n_rows=2, hidden=hidden, capture=cap.data_ptr(), ld_cap=ld,
                vec=vec.data_ptr(), ld_vec=ld, mode=1, alpha=0.5)

    def call(**kw):
        a = dict(base, **kw)
        return lib.icl_resid_rows_f32(a["h"], a["ldh"], a["rows"], a["n_rows"], a["hidden"], a["capture"], a["ld_cap"], a["vec"],
                                      a["ld_vec"], a["mode"], a["alpha"], st)
    refusals = {
        "h is NULL": dict(h=0), "rows is NULL": dict(rows=0), "both NULL": dict(capture=0, vec=0),
        "n_rows": [dict(n_rows=0), dict(n_rows=65536), dict(n_rows=-1)],
        "hidden": [dict(hidden=0), dict(hidden=6), dict(hidden=-4)],
        "ldh": [dict(ldh=4), dict(ldh=18)], "ld_cap": [dict(ld_cap=4), dict(ld_cap=18)], "ld_vec": [dict(ld_vec=4), dict(ld_vec=18)],
        "h is not 16-byte": dict(h=h.data_ptr() + 4), "capture is not 16-byte": dict(capture=cap.data_ptr() + 8),
        "vec is not 16-byte": dict(vec=vec.data_ptr() + 4),
        "mode": [dict(mode=2), dict(mode=-1)], "alpha": [dict(alpha=float("nan")), dict(alpha=float("inf"))],
    }
    for word, kws in refusals.items():
        for kw in (kws if isinstance(kws, list) else [kws]):
            assert call(**kw) == -1, (word, kw)
            msg = lib.icl_last_error().decode()
            assert msg.startswith("icl_resid_rows_f32") and word in msg, (word, msg)
    # the same through the binding: an IclError naming the entry point and the argument
    for word, kw in {"n_rows": dict(rows=torch.zeros(65536, dtype=I32, device=DEV), capture=torch.zeros(65536, hidden, device=DEV), vec=vec[0, :hidden]),
                     "hidden": dict(hidden=6), "mode": dict(mode=2), "alpha": dict(alpha=float("inf")),
                     "both NULL": dict(capture=None, vec=None), "16-byte": dict(h=h[:, 1:1 + hidden])}.items():
        a = dict(dict(h=h[:, :hidden], rows=rows, capture=cap[:, :hidden], vec=vec[:, :hidden], mode="add", alpha=0.5, hidden=hidden), **kw)
        with pytest.raises(B.IclError, match="icl_resid_rows_f32.*" + word):
            B.resid_rows(a["h"], a["rows"], capture=a["capture"], vec=a["vec"], mode=a["mode"], alpha=a["alpha"], hidden=a["hidden"])
    with pytest.raises(B.IclError, match="GPU"):
        B.resid_rows(h.cpu(), rows, capture=cap)
    torch.cuda.synchronize()
    for t, b in zip((h, cap, vec), before):
        assert torch.equal(t, b)
    assert call() == 0                                                            # the valid call, last
    torch.cuda.synchronize()
    assert torch.equal(cap[:, :hidden], before[0][[1, 3], :hidden]) and torch.equal(h[1, :hidden], before[0][1, :hidden] + 2.5)
    assert torch.equal(h[:, hidden:], before[0][:, hidden:]) and torch.equal(h[0], before[0][0])

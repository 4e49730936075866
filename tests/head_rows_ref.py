"""Support for the head-output tests (tests/test_head_rows_ref.py on the CPU, tests/test_gpu_head_rows.py on the GPU): not a test
module.

icl_head_rows_bf16 (include/icl_hip.h): a float64 reference of one launch (``expect``), the assertions every test applies to a
launch's result (``check``), an f32 emulation in the kernel's order with one-mistake mutants (``emulate``), the table of launches
(``launch_cases``) shared by the CPU and the GPU module, and the far-offset case (``far_case``).

What is compared how.  Capture, unlisted rows, unselected heads and the pad columns: as bits.  Replace: as bits against
bf16_rne(v) (tests/fp64_bounds.py) — for a v that is a bf16 value, NaN payloads included, that is v's upper 16 bits.  Add: the
kernel computes bf16(fl32(alpha * v + a)); the reference is ref = fl64(p + a) of the exact product p = alpha * v (24 x 24 bits fit
53), and the f32 value is ONE rounding of the exact sum, within e = 2^-24 |ref| + 2^-149 of ref (the second term: half a subnormal
step, where the relative term vanishes), so the bf16 output lies in ``bf16_interval(ref, e)`` — no added output ulp, no new
tolerance.  The cancellation probe a = -bf16-value, v = fl32(-a / alpha): the fused form leaves the rounding error of the
product, a value some 2^-24 |a|; multiply-then-add leaves 0 or a whole f32 ulp of a, which the interval around that residual
does not hold."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import far_layout as fl
from fp64_bounds import bf16_interval, bf16_rne, in_interval, interval_ratio
from resid_patch_ref import fma32, keyed_rng

SHAPES = ((64, 3), (128, 4), (128, 40))    # (head_dim, n_heads): 8 and 16 lanes per head row; one block, part of one, two and a half
N_ROWS = (1, 3, 65)
ROWS_TOTAL = 70
PAD = 8                                    # ld_att = n_heads * head_dim + PAD: att is a column slice of a wider, sentinel-filled buffer
SENTINEL = 0x7FA5                          # a bf16 NaN bit pattern no launch writes
SELECTIONS = ("one", "two", "all")         # n_sel 1, 2 (unsorted) and n_heads
MUTANTS = ("head_plus_1", "next_head_vector", "row_plus_1", "shared_vector", "capture_after", "add_as_replace", "mul_then_add",
           "whole_row")
SPECIALS = np.array([0x7FC1, 0xFFC3, 0x7F81, 0x8000, 0x0000, 0x7F80, 0xFF80, 0x0001, 0x807F, 0x0040, 0x7F7F, 0xFF7F],
                    dtype=np.uint16)       # NaN payloads (quiet and signalling), -0.0, 0, +-inf, subnormals, +-max


@dataclass(frozen=True)
class Launch:
    D: int
    H: int
    n_rows: int
    sel: str                    # key of SELECTIONS
    capture: bool
    mode: Optional[str]         # None (no patch) | "replace" | "add"
    shared: bool = False        # one block of vectors for all entries
    data: str = "bits"          # "bits" (special values everywhere, bf16-valued vectors) | "normal" | "tiny" | "huge" | "cancel"
    alpha: float = 1.0
    reverse: bool = False       # the list in reverse order (with its vectors): the same bits

    @property
    def id(self):
        return (f"D{self.D}-H{self.H}-n{self.n_rows}-{self.sel}-{'cap' if self.capture else 'nocap'}-{self.mode}-"
                f"{'shared' if self.shared else 'perrow'}-{self.data}{'-rev' if self.reverse else ''}")

    @property
    def width(self):
        return self.H * self.D


def heads_of(c: Launch) -> np.ndarray:
    """Distinct heads of the launch's selection (the head + 1 mutant wraps around inside the row)."""
    if c.sel == "one":
        return np.array([c.H - 2], dtype=np.int32)
    if c.sel == "two":
        return np.array([2, 0], dtype=np.int32)             # unsorted
    return keyed_rng("heads", c.H).permutation(c.H).astype(np.int32)


def launch_cases(D, H, n_rows):
    """The launches of one (head_dim, n_heads, n_rows) shape: capture only; for every selection patch only and both, per-row and
    shared vectors, replace of bf16-valued and of arbitrary f32 vectors, add on the four kinds of data."""
    out = [Launch(D, H, n_rows, "one", True, None)]
    for sel in SELECTIONS:
        for cap in (False, True):
            for shared in (False, True):
                out.append(Launch(D, H, n_rows, sel, cap, "replace", shared))
                out.append(Launch(D, H, n_rows, sel, cap, "replace", shared, "normal"))
                kinds = (("normal", 0.7), ("cancel", 0.7)) if shared else (("normal", 0.7), ("tiny", -1.3), ("huge", 3.1), ("cancel", 0.7))
                for data, alpha in kinds:
                    out.append(Launch(D, H, n_rows, sel, cap, "add", shared, data, alpha))
    return out


def rows_of(c: Launch):
    """Distinct rows of the 70, never the last one (a row + 1 mutant stays inside), in no particular order."""
    rows = keyed_rng("rows", c.n_rows).permutation(ROWS_TOTAL - 1)[:c.n_rows].astype(np.int32)
    return rows[::-1].copy() if c.reverse else rows


def _bf16_bits(x: np.ndarray) -> np.ndarray:
    """f32 array -> the uint16 bits of its round-to-nearest-even bf16 (finite values)."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def widen(bits: np.ndarray) -> np.ndarray:
    """bf16 bits (uint16) -> the f32 values they stand for."""
    return (bits.astype(np.uint32) << 16).view(np.float32)


def inputs(c: Launch):
    """(att uint16 [70, width + PAD] bf16 bits with the sentinel in the PAD columns, rows int32 [n], heads int32 [n_sel] | None,
    vec f32 [n or 1, n_sel, D] | None)."""
    g = keyed_rng("data", c.D, c.H, c.n_rows, c.sel, c.data, c.shared)
    heads = heads_of(c)
    nv, ns = (1 if c.shared else c.n_rows), len(heads)
    if c.data == "bits":
        a = _bf16_bits(g.standard_normal((ROWS_TOTAL, c.width)).astype(np.float32)).copy()
        v = _bf16_bits(g.standard_normal((nv * ns, c.D)).astype(np.float32)).copy()
        for x in (a, v):                                   # specials over a third of the elements, all of them in every row
            m = g.random(x.shape) < 1 / 3
            x[m] = SPECIALS[g.integers(0, len(SPECIALS), int(m.sum()))]
            x[:, :len(SPECIALS)] = SPECIALS[(5 * np.arange(x.shape[0])[:, None] + np.arange(len(SPECIALS))[None] + (x is v)) % len(SPECIALS)]
        v = widen(v).reshape(nv, ns, c.D)                  # bf16-valued f32, NaN payloads and subnormals among them
    else:
        scale = {"normal": 1.0, "tiny": 2.0 ** -20, "huge": 2.0 ** 20, "cancel": 1.0}[c.data]
        a = _bf16_bits((g.standard_normal((ROWS_TOTAL, c.width)) * scale).astype(np.float32)).copy()
        v = (g.standard_normal((nv, ns, c.D)) * scale).astype(np.float32)
    rows = rows_of(c)
    if c.reverse and not c.shared:                          # entry r of the reversed list carries the vectors of the same row
        v = v[::-1].copy()
    if c.data == "cancel":                                  # alpha * v = -a up to the product's rounding, on the selected heads
        al = np.float32(c.alpha)
        for r, row in enumerate(rows if not c.shared else rows[:1]):
            for s, h in enumerate(heads):
                av = widen(a[row, h * c.D:(h + 1) * c.D])
                v[0 if c.shared else r, s] = (-av.astype(np.float64) / np.float64(al)).astype(np.float32)
        if c.shared:                                        # one block for all entries: every listed row holds the first one's heads
            for row in rows[1:]:
                for h in heads:
                    a[row, h * c.D:(h + 1) * c.D] = a[rows[0], h * c.D:(h + 1) * c.D]
    full = np.full((ROWS_TOTAL, c.width + PAD), SENTINEL, dtype=np.uint16)
    full[:, :c.width] = a
    return full, rows, (heads if c.mode is not None else None), (v if c.mode is not None else None)


@dataclass
class Expect:
    bits: np.ndarray                   # uint16 [70, ld]: what every element that is compared as bits must hold
    exact: np.ndarray                  # bool   [70, ld]: the elements compared as bits (all but the selected heads of an add)
    add_ref: Optional[np.ndarray]      # f64 [n, n_sel, D] | None
    cap_bits: Optional[np.ndarray]     # uint16 [n, width] | None
    rows: np.ndarray
    heads: Optional[np.ndarray]


def _replace_bits(v: np.ndarray) -> np.ndarray:
    """bf16_rne of the f32 vectors as bits; a bf16-valued v (NaN payloads included) is its upper half."""
    vb = v.view(np.uint32)
    valued = (vb & 0xFFFF) == 0
    rne = bf16_rne(torch.from_numpy(np.where(valued, np.float32(0), v).astype(np.float64))).float().numpy().view(np.uint32) >> 16
    return np.where(valued, vb >> 16, rne).astype(np.uint16)


def expect(c: Launch, att, rows, heads, vec) -> Expect:
    """The float64 reference of the launch on ``inputs(c)``."""
    bits = att.copy()
    exact = np.ones(bits.shape, dtype=bool)
    cap = att[rows, :c.width].copy() if c.capture else None
    add = None
    if c.mode is not None:
        if c.mode == "add":
            add = np.zeros((c.n_rows, len(heads), c.D))
        for r, row in enumerate(rows):
            for s, h in enumerate(heads):
                v, sl = vec[0 if c.shared else r, s], slice(h * c.D, (h + 1) * c.D)
                if c.mode == "replace":
                    bits[row, sl] = _replace_bits(v)
                else:
                    add[r, s] = np.float64(np.float32(c.alpha)) * v.astype(np.float64) + widen(att[row, sl]).astype(np.float64)
                    exact[row, sl] = False
    return Expect(bits, exact, add, cap, rows, heads)


def add_error(ref):
    """e of ``bf16_interval(ref, e)``: the one f32 rounding of the exact alpha * v + a."""
    return 2.0 ** -24 * ref.abs() + 2.0 ** -149


def check(c: Launch, e: Expect, att_out, cap_out):
    """The assertions on one launch's result (att_out uint16 [70, ld], cap_out uint16 [n, width] | None): the list of what fails,
    and the largest ``interval_ratio`` of an add."""
    fails, worst = [], 0.0
    bad = (att_out != e.bits) & e.exact
    if bad.any():
        r, i = np.argwhere(bad)[0]
        fails.append(f"{int(bad.sum())} elements of att differ in bits, first at row {r} column {i} (head {i // c.D})")
    if c.capture:
        if cap_out is None or not np.array_equal(cap_out, e.cap_bits):
            fails.append("capture is not the pre-patch rows, bit for bit")
    if e.add_ref is not None:
        out = np.stack([np.stack([widen(att_out[row, h * c.D:(h + 1) * c.D]) for h in e.heads]) for row in e.rows])
        out, ref = torch.from_numpy(out), torch.from_numpy(e.add_ref)
        lo, hi = bf16_interval(ref, add_error(ref))
        ok = in_interval(out, lo, hi)
        if not bool(ok.all()):
            fails.append(f"add: {int((~ok).sum())} elements outside bf16_interval(ref, 2^-24 |ref| + 2^-149)")
        worst = interval_ratio(out, ref, lo, hi)
    return fails, worst


def emulate(c: Launch, att, rows, heads, vec, mutant=None):
    """The kernel in f32 on the CPU (a thread: one 16-byte chunk of entry r's row rows[r]; its loads, then the capture store, then
    the att store), or one of MUTANTS.  -> (att_out uint16 [70, ld], cap uint16 [n, width] | None)."""
    assert mutant is None or mutant in MUTANTS
    out = att.copy()
    cap = np.zeros((c.n_rows, c.width), dtype=np.uint16) if c.capture else None
    al = np.float32(c.alpha)
    for r, row in enumerate(rows):
        row = int(row) + (mutant == "row_plus_1")
        x = att[row, :c.width].copy()
        new = x.copy()
        if c.mode is not None:
            targets = [(s, int(h)) for s, h in enumerate(heads)]
            if mutant == "head_plus_1":
                targets = [(s, (h + 1) % c.H) for s, h in targets]
            if mutant == "whole_row":
                targets = [(0, h) for h in range(c.H)]
            for s, h in targets:
                vr = 0 if (c.shared or mutant == "shared_vector") else r
                vs = (s + 1) % len(heads) if mutant == "next_head_vector" else s
                v, sl = vec[vr, vs], slice(h * c.D, (h + 1) * c.D)
                if c.mode == "replace" or mutant == "add_as_replace":      # the kernel's select: a bf16-valued v is its upper half
                    vb = v.view(np.uint32)
                    new[sl] = np.where((vb & 0xFFFF) == 0, (vb >> 16).astype(np.uint16), _bf16_bits(np.where(np.isnan(v), np.float32(0), v)))
                elif mutant == "mul_then_add":
                    new[sl] = _bf16_bits((al * v).astype(np.float32) + widen(x[sl]))
                else:
                    new[sl] = _bf16_bits(fma32(np.full_like(v, al), v, widen(x[sl])))
            out[row, :c.width] = new
        if c.capture:
            cap[r] = new if mutant == "capture_after" else x
    return out, cap


def mutant_applies(mutant, c: Launch) -> bool:
    """Whether the mistake changes anything a launch of this kind could show."""
    if mutant == "row_plus_1":
        return True
    if c.mode is None:
        return False
    if mutant == "head_plus_1":
        return True
    if mutant == "next_head_vector":
        return c.sel != "one"
    if mutant == "whole_row":
        return c.sel != "all"
    if mutant == "shared_vector":
        return not c.shared and c.n_rows > 1
    if mutant == "capture_after":
        return c.capture
    if mutant == "add_as_replace":
        return c.mode == "add"
    return c.mode == "add" and c.data == "cancel"           # mul_then_add: shown by the cancellation probe


# ------------------------------------------------------------------------------------------------------------------
# the far-offset case
# ------------------------------------------------------------------------------------------------------------------
FAR_D, FAR_H = 128, 4


def far_case():
    """att rows 0 and 1 at a leading dimension of 2^32 + 64 elements (row 1 starts beyond 8 GiB, beyond 2^32 elements); capture
    and the per-row vectors stay near.  Capture + add of all heads: every operand is read or written at the far row."""
    n = FAR_D * FAR_H
    ops = [fl.stride_op("att", "bf16", "inout", n), fl.plain_op("capture", "bf16", "out", n, 2), fl.plain_op("vec", "f32", "in", n, 2)]
    return fl.place(fl.Case("head_rows", "head", "stride", ops, dict(head_dim=FAR_D, n_heads=FAR_H)))

"""Support for the residual-stream tests (tests/test_resid_patch_ref.py on the CPU, tests/test_gpu_resid_patch.py on the GPU): not
a test module.

1. icl_resid_rows_f32 (include/icl_hip.h): a float64 reference of one launch (``expect``), the assertions every test applies to a
   launch's result (``check``), an f32 emulation of the kernel with one-mistake mutants (``emulate``), and the table of launches
   (``launch_cases``) shared by the CPU and the GPU module.

   The bound for add.  The kernel computes fl32(alpha * v + h), ONE rounding of the exact value x: |out - x| <= 2^-24 |x| when x is
   in the normal range, and <= 2^-150 (half a subnormal step) below it.  The reference is the float64 sum ref = fl64(p + h) of the
   exact product p = alpha * v (24 x 24 bits fit 53), so |ref - x| <= 2^-53 |x|.  Together, with |x| <= (1 + 2^-53) |ref|:
       |out - ref| <= 2^-24 |x| + 2^-53 |x| <= (2^-24 + 2^-50) |ref| + 2^-126,
   the 2^-126 covering the subnormal range with room to spare.  Capture, replace, unlisted rows and the columns beyond ``hidden``
   are compared as bits.  The cancellation probe h = -fl32(alpha * v): the fused form returns the rounding error of the product,
   exactly (non-zero wherever the product was inexact); multiply-then-add returns 0, which misses ref by |ref| — refused.

2. The far-offset case (tests/far_layout.py): ldh = 2^32 + 64, rows 0 and 1.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

import far_layout as fl

# ------------------------------------------------------------------------------------------------------------------
# 1. the launch
# ------------------------------------------------------------------------------------------------------------------
HIDDENS = (4, 1020, 1024, 1028, 5120)      # one lane, one short of a pass, exactly one pass, one lane into the second pass, several
N_ROWS = (1, 3, 65)
ROWS_TOTAL = 70
PAD = 8                                    # ldh = hidden + PAD: h is a column slice of a wider, sentinel-filled buffer
SENTINEL = 0x7FA5C3E1                      # a NaN bit pattern no launch writes
REL, ABS = 2.0 ** -24 + 2.0 ** -50, 2.0 ** -126
MUTANTS = ("mul_then_add", "row_plus_1", "next_vector", "shared_vector", "capture_after", "add_as_replace")
SPECIALS = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF,
                     0x00400000, 0x7F7FFFFF, 0xFF7FFFFF], dtype=np.uint32)   # NaN payloads, -0.0, 0, +-inf, subnormals, +-max


@dataclass(frozen=True)
class Launch:
    hidden: int
    n_rows: int
    capture: bool
    mode: Optional[str]         # None (no patch) | "replace" | "add"
    shared: bool = False        # one vector for all entries
    data: str = "bits"          # "bits" (special values everywhere) | "normal" | "tiny" (x 2^-20) | "huge" (x 2^20) | "cancel"
    alpha: float = 1.0
    reverse: bool = False       # the list in reverse order (with its vectors): the same bits

    @property
    def id(self):
        return (f"h{self.hidden}-n{self.n_rows}-{'cap' if self.capture else 'nocap'}-{self.mode}-{'shared' if self.shared else 'perrow'}-"
                f"{self.data}{'-rev' if self.reverse else ''}")


def launch_cases(hidden, n_rows):
    """The launches of one (hidden, n_rows) shape: capture only, patch only, both; shared and per-row vectors; add on the four
    kinds of data."""
    out = [Launch(hidden, n_rows, True, None)]
    for cap in (False, True):
        for shared in (False, True):
            out.append(Launch(hidden, n_rows, cap, "replace", shared))
            for data, alpha in (("normal", 0.7), ("tiny", -1.3), ("huge", 3.1), ("cancel", 0.7)):
                out.append(Launch(hidden, n_rows, cap, "add", shared, data, alpha))
    return out


def keyed_rng(*key):
    import zlib
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def rows_of(c: Launch):
    """Distinct rows of the 70, never the last one (a row + 1 mutant stays inside), in no particular order."""
    rows = keyed_rng("rows", c.n_rows).permutation(ROWS_TOTAL - 1)[:c.n_rows].astype(np.int32)
    return rows[::-1].copy() if c.reverse else rows


def inputs(c: Launch):
    """(h f32 [70, hidden + PAD] with the sentinel in the PAD columns, rows int32 [n], vec f32 [n or 1, hidden] | None)."""
    g = keyed_rng("data", c.hidden, c.n_rows, c.data, c.shared)
    nv = 1 if c.shared else c.n_rows
    if c.data == "bits":
        h = g.standard_normal((ROWS_TOTAL, c.hidden)).astype(np.float32).view(np.uint32)
        v = g.standard_normal((nv, c.hidden)).astype(np.float32).view(np.uint32)
        for a in (h, v):                                   # specials over a third of the elements, all of them in every row
            m = g.random(a.shape) < 1 / 3
            a[m] = SPECIALS[g.integers(0, len(SPECIALS), int(m.sum()))]
            k = min(c.hidden, len(SPECIALS))               # ... rotated by the row, so that no two neighbouring rows are alike
            a[:, :k] = SPECIALS[(5 * np.arange(a.shape[0])[:, None] + np.arange(k)[None] + (a is v)) % len(SPECIALS)]
        h, v = h.view(np.float32), v.view(np.float32)
    else:
        scale = {"normal": 1.0, "tiny": 2.0 ** -20, "huge": 2.0 ** 20, "cancel": 1.0}[c.data]
        h = (g.standard_normal((ROWS_TOTAL, c.hidden)) * scale).astype(np.float32)
        v = (g.standard_normal((nv, c.hidden)) * scale).astype(np.float32)
    rows = rows_of(c)
    if c.reverse and not c.shared:                          # entry r of the reversed list carries the vector of the same row
        v = v[::-1].copy()
    if c.data == "cancel":                                  # h = -fl32(alpha * v) on the listed rows
        a = np.float32(c.alpha)
        for r, row in enumerate(rows):
            h[row] = -(a.astype(np.float64) * v[0 if c.shared else r].astype(np.float64)).astype(np.float32)
    full = np.full((ROWS_TOTAL, c.hidden + PAD), SENTINEL, dtype=np.uint32)
    full[:, :c.hidden] = h.view(np.uint32)
    return full.view(np.float32), rows, (v if c.mode is not None else None)


@dataclass
class Expect:
    h_bits: np.ndarray                 # uint32 [70, ld]: what every element that is compared as bits must hold
    exact: np.ndarray                  # bool   [70, ld]: the elements compared as bits (all but the listed rows of an add)
    add_ref: Optional[np.ndarray]      # f64 [n, hidden] | None
    cap_bits: Optional[np.ndarray]     # uint32 [n, hidden] | None
    rows: np.ndarray


def expect(c: Launch, h, rows, vec) -> Expect:
    """The float64 reference of the launch on ``inputs(c)``."""
    hb = h.view(np.uint32).copy()
    exact = np.ones(hb.shape, dtype=bool)
    cap = hb[rows, :c.hidden].copy() if c.capture else None
    add = None
    if c.mode == "replace":
        for r, row in enumerate(rows):
            hb[row, :c.hidden] = vec[0 if c.shared else r].view(np.uint32)
    elif c.mode == "add":
        a = np.float64(np.float32(c.alpha))
        add = np.stack([a * vec[0 if c.shared else r].astype(np.float64) + h[row, :c.hidden].astype(np.float64)
                        for r, row in enumerate(rows)])
        exact[rows, :c.hidden] = False
    return Expect(hb, exact, add, cap, rows)


def check(c: Launch, e: Expect, h_out, cap_out) -> list:
    """The assertions on one launch's result (h_out f32 [70, ld], cap_out f32 [n, hidden] | None): the list of what fails, and
    the largest |out - ref| / bound of an add."""
    fails, worst = [], 0.0
    got = h_out.view(np.uint32)
    bad = (got != e.h_bits) & e.exact
    if bad.any():
        r, i = np.argwhere(bad)[0]
        kind = "a listed row" if r in set(e.rows.tolist()) and i < c.hidden else "outside the listed rows' first hidden columns"
        fails.append(f"{int(bad.sum())} elements of h differ in bits, first at row {r} column {i} ({kind})")
    if c.capture:
        if cap_out is None or not np.array_equal(cap_out.view(np.uint32), e.cap_bits):
            fails.append("capture is not the pre-patch rows, bit for bit")
    if e.add_ref is not None:
        out = h_out[e.rows, :c.hidden].astype(np.float64)
        err, bound = np.abs(out - e.add_ref), REL * np.abs(e.add_ref) + ABS
        if not np.isfinite(out).all() or (err > bound).any():
            fails.append(f"add: |out - ref| exceeds (2^-24 + 2^-50) |ref| + 2^-126 at {int((~(err <= bound)).sum())} elements")
        worst = float((err / bound).max())
    return fails, worst


def fma32(a, v, h):
    """fl32(a * v + h) with ONE rounding, for finite f32 arrays: the product is exact in f64; the f64 sum is taken with round-to-odd
    (TwoSum gives its exact error), which a second rounding to 24 bits cannot turn into a double rounding."""
    p = a.astype(np.float64) * v.astype(np.float64)
    h = h.astype(np.float64)
    s = p + h
    bb = s - p
    err = (p - (s - bb)) + (h - bb)
    odd = (s.view(np.uint64) & np.uint64(1)).astype(bool)
    fix = (err != 0) & ~odd
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def emulate(c: Launch, h, rows, vec, mutant=None):
    """The kernel in f32 on the CPU (block r: row rows[r], vector r or the shared one; loads, then the capture store, then the h
    store), or one of MUTANTS.  -> (h_out f32 [70, ld], cap f32 [n, hidden] | None)."""
    assert mutant is None or mutant in MUTANTS
    out = h.copy()
    cap = np.zeros((c.n_rows, c.hidden), dtype=np.float32) if c.capture else None
    a = np.float32(c.alpha)
    for r, row in enumerate(rows):
        row = int(row) + (mutant == "row_plus_1")
        x = h[row, :c.hidden].copy()
        new = None
        if c.mode is not None:
            vr = 0 if c.shared else r
            if mutant == "next_vector":
                vr = (r + 1) % vec.shape[0]
            if mutant == "shared_vector":
                vr = 0
            v = vec[vr]
            if c.mode == "replace" or mutant == "add_as_replace":
                new = v.copy()
            elif mutant == "mul_then_add":
                new = (a * v).astype(np.float32) + x
            else:
                new = fma32(np.full_like(v, a), v, x)
            out[row, :c.hidden] = new
        if c.capture:
            cap[r] = new if (mutant == "capture_after" and new is not None) else x
    return out, cap


def mutant_applies(mutant, c: Launch) -> bool:
    """Whether the mistake changes anything a launch of this kind could show."""
    if mutant == "row_plus_1":
        return True
    if c.mode is None:
        return False
    if mutant in ("next_vector", "shared_vector"):
        return not c.shared and c.n_rows > 1
    if mutant == "capture_after":
        return c.capture
    if mutant == "add_as_replace":
        return c.mode == "add"
    return c.mode == "add" and c.data == "cancel"           # mul_then_add: shown by the cancellation probe


# ------------------------------------------------------------------------------------------------------------------
# 2. the far-offset case
# ------------------------------------------------------------------------------------------------------------------
FAR_HIDDEN = 1028


def far_case():
    """h rows 0 and 1 at a leading dimension of 2^32 + 64 elements (row 1 starts beyond 16 GiB); capture and the per-row vectors
    stay near.  Capture + add: every operand is read or written at the far row."""
    n = FAR_HIDDEN
    ops = [fl.stride_op("h", "f32", "inout", n), fl.plain_op("capture", "f32", "out", n, 2), fl.plain_op("vec", "f32", "in", n, 2)]
    return fl.place(fl.Case("resid_rows", "resid", "stride", ops, dict(hidden=n)))

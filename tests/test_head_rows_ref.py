"""Attention-head output capture and patching, without a GPU: the float64 reference and the assertions of tests/head_rows_ref.py
admit an f32 emulation of icl_head_rows_bf16 in the kernel's order on every launch of the table, and reject eight one-mistake
mutants on every launch that could show the mistake: the head heads[s] + 1, the next selected head's vector, row rows[r] + 1, the
shared vector used for per-row ones, a capture taken after the patch, add performed as replace, add with the product rounded before
the sum (on the cancellation probe) and the whole row written where some heads are selected.  The far-offset case keeps every
32-bit narrowing inside the arena and inside a compared window."""
import numpy as np
import pytest

import far_layout as fl
import head_rows_ref as hr

SHAPES = [(D, H, n) for D, H in hr.SHAPES for n in hr.N_ROWS]
IDS = [f"D{D}-H{H}-n{n}" for D, H, n in SHAPES]


@pytest.mark.parametrize("D,H,n_rows", SHAPES, ids=IDS)
def test_the_emulation_passes_and_every_mutant_is_rejected(D, H, n_rows):
    tried = {m: 0 for m in hr.MUTANTS}
    worst_all = 0.0
    for c in hr.launch_cases(D, H, n_rows):
        args = hr.inputs(c)
        e = hr.expect(c, *args)
        fails, worst = hr.check(c, e, *hr.emulate(c, *args))
        assert not fails and worst <= 1.0, (c.id, fails, worst)
        worst_all = max(worst_all, worst)
        for m in hr.MUTANTS:
            if hr.mutant_applies(m, c):
                tried[m] += 1
                fails, _ = hr.check(c, e, *hr.emulate(c, *args, mutant=m))
                assert fails, f"{c.id}: mutant {m} passes"
    assert all(n > 0 for m, n in tried.items() if n_rows > 1 or m != "shared_vector"), tried
    print(f"head_rows D {D} H {H} n_rows {n_rows}: emulation, largest interval ratio {worst_all:.3f}")


def test_the_cancellation_probe_separates_fused_from_multiply_then_add():
    c = hr.Launch(128, 4, 3, "two", False, "add", False, "cancel", 0.7)
    att, rows, heads, vec = hr.inputs(c)
    fused, _ = hr.emulate(c, att, rows, heads, vec)
    split, _ = hr.emulate(c, att, rows, heads, vec, mutant="mul_then_add")
    cols = np.concatenate([np.arange(h * c.D, (h + 1) * c.D) for h in heads])
    f, s, a = (hr.widen(x[rows][:, cols]) for x in (fused, split, att))
    assert (f != 0).mean() > 0.5 and (np.abs(f) <= 2.0 ** -23 * np.abs(a)).all()      # the product's rounding error, not zero
    assert ((s == 0) | (np.abs(s) >= 2.0 ** -24 * np.abs(a))).all() and (s != f).mean() > 0.5


def test_replace_of_a_bf16_value_is_its_bits_and_of_any_f32_its_nearest_even():
    c = hr.Launch(64, 3, 3, "all", False, "replace", False, "bits")
    att, rows, heads, vec = hr.inputs(c)
    out, _ = hr.emulate(c, att, rows, heads, vec)
    for r, row in enumerate(rows):
        for s, h in enumerate(heads):
            assert np.array_equal(out[row, h * 64:(h + 1) * 64], (vec[r, s].view(np.uint32) >> 16).astype(np.uint16))
    assert np.isnan(vec).any() and (vec.view(np.uint32) == 0x80000000).any()
    x = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0], dtype=np.float32)    # two ties, one above, exact
    assert hr._replace_bits(x).tolist() == [0x3F80, 0x3F82, 0x3F81, 0xC040]


@pytest.mark.parametrize("mode", ["replace", "add"])
def test_a_list_and_its_reverse_give_the_same_bits(mode):
    base = hr.Launch(128, 4, 65, "two", True, mode, False, "bits" if mode == "replace" else "normal", 0.7)
    outs = []
    for c in (base, hr.Launch(**{**base.__dict__, "reverse": True})):
        att, rows, heads, vec = hr.inputs(c)
        out, cap = hr.emulate(c, att, rows, heads, vec)
        outs.append((att, rows, out, cap))
    (a0, r0, o0, c0), (a1, r1, o1, c1) = outs
    assert np.array_equal(a0, a1) and np.array_equal(r0, r1[::-1])
    assert np.array_equal(o0, o1) and np.array_equal(c0, c1[::-1]) and not np.array_equal(o0, a0)


def test_far_case_every_narrowing_lands_inside_the_arena_and_a_compared_window():
    case = hr.far_case()
    assert case.op("att").is_far() and case.op("att").meta["ld"] == fl.LD_FAR == 2 ** 32 + 64
    wins = sorted((o.base + lo, o.base + hi, o.name) for o in case.ops for lo, hi in o.windows())
    for (lo0, hi0, n0), (lo1, hi1, n1) in zip(wins, wins[1:]):
        assert hi0 <= lo1, f"windows of {n0} and {n1} overlap"
    for o in case.ops:
        assert o.base >= fl.MARGIN and o.base % 256 == 0
        nb = o.n * o.esize
        for off, tw in zip(o.offs, o.twin):
            assert (off * o.esize) % 128 == (tw * o.esize) % 128
            for kind in (None,) + fl.NARROWINGS:
                lo = fl.narrow(off, o.esize, kind)
                assert fl.narrow(off + o.n - 1, o.esize, kind) == lo + nb - o.esize, "a row straddles a 32-bit wrap"
                assert 0 <= o.base + lo - fl.MARGIN and o.base + lo + nb + fl.MARGIN <= fl.ARENA_BYTES, (o.name, off, kind)
                assert any(w0 + fl.MARGIN <= lo and lo + nb <= w1 - fl.MARGIN for w0, w1 in o.windows()), (o.name, off, kind)
        assert o.meta["ld"] % 8 == 0 and o.meta["ld_twin"] % 8 == 0 and o.meta["ld_twin"] >= o.n
    # a narrowed leading dimension puts row 1 of att 64 elements after row 0: inside row 0's window, where the twin comparison sees it
    a = case.op("att")
    assert {fl.narrow(a.offs[1], 2, k) for k in fl.NARROWINGS} == {64 * 2}

"""The layout of tests/test_gpu_far_offsets.py, checked without a GPU: every far-offset case keeps every 32-bit narrowing of every
address inside the arena and inside a window the GPU test compares, and the GPU test's assertions reject a launch that narrows
(a numpy model of the launch over a sparse dict of those windows; the idea of tests/test_attention_probes.py)."""
import pytest

import far_layout as fl

CASES = fl.CASES
IDS = [c.name for c in CASES]


def _abs_windows(case):
    return [(o.base + lo, o.base + hi, o.name) for o in case.ops for lo, hi in o.windows()]


def test_the_table_names_every_group():
    assert {c.group for c in CASES} == {"norm", "rope", "glue", "tail", "gemm", "gemm_rmsnorm", "gemm_batched", "decode", "decode_gqa", "decode_fp8",
                                        "decode_rope", "kv_copy", "qformer", "prefill", "prefill_cache", "gemm_rope", "segmass", "frontend"}
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_case_reaches_2_pow_32_elements(case):
    far = [o for o in case.ops if o.is_far()]
    assert far, "no operand of this case has a row at or beyond 2^32 elements of its own type"
    for o in case.ops:
        assert o.base >= fl.MARGIN and o.base % 256 == 0
        assert len(o.offs) == len(o.twin) and len(set(o.offs)) == len(o.offs)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_narrowing_leaves_the_arena(case):
    """True place and all four narrowings of the first and the last element of every row, margins included."""
    for o in case.ops:
        nb = o.n * o.esize
        for off in o.offs:
            for kind in (None,) + fl.NARROWINGS:
                lo = fl.narrow(off, o.esize, kind)
                assert fl.narrow(off + o.n - 1, o.esize, kind) == lo + nb - o.esize, f"{o.name}: a row straddles a 32-bit wrap ({kind})"
                assert 0 <= o.base + lo - fl.MARGIN and o.base + lo + nb + fl.MARGIN <= fl.ARENA_BYTES, (o.name, off, kind)


@pytest.mark.parametrize("case", [c for c in CASES if "geom" in c.p], ids=[c.name for c in CASES if "geom" in c.p])
def test_grid_walk_every_sequence_stays_inside(case):
    """The launch walks ALL sequences, not only the compared ones: the one position an unchecked sequence reads, under every
    narrowing.  This is what forces the operand's base 2^31 elements above the arena's start."""
    seq_elems, nseq = case.p["geom"]
    assert (nseq - 3) * seq_elems >= fl.FAR and any(1 << 31 <= s * seq_elems < fl.FAR for s in fl.grid_checked(case.p["geom"]))
    for o in case.ops:
        if "seq_elems" not in o.meta:               # an fp8 scale plane: [n_seqs][max_len] f32 beside its byte plane, below 2^31 bytes
            assert max(o.offs) * o.esize < 1 << 31
            continue
        assert o.base >= (1 << 31) * o.esize + fl.MARGIN
        for b in range(nseq):
            for kind in (None,) + fl.NARROWINGS:
                lo = o.base + fl.narrow(b * seq_elems, o.esize, kind)
                assert 0 <= lo and lo + fl.GRID_ROWS * case.p["D"] * o.esize <= fl.ARENA_BYTES, (o.name, b, kind)


@pytest.mark.parametrize("case", [c for c in CASES if "geom" not in c.p], ids=[c.name for c in CASES if "geom" not in c.p])
def test_stride_and_index_offsets_narrow_to_small_non_negative_numbers(case):
    """Offsets are 2^32 k + d with d * esize < 2^31 (or below 2^31 bytes altogether), so every narrowing is a small non-negative
    number: nothing lands below the operand's pointer."""
    for o in case.ops:
        for off in o.offs:
            d = off % fl.FAR
            assert d * o.esize < 1 << 31, (o.name, off)
            for kind in fl.NARROWINGS:
                assert 0 <= fl.narrow(off, o.esize, kind) < 1 << 31, (o.name, off, kind)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_operands_share_the_arena_at_disjoint_windows(case):
    wins = sorted(_abs_windows(case))
    for (lo0, hi0, n0), (lo1, hi1, n1) in zip(wins, wins[1:]):
        assert hi0 <= lo1, f"windows of {n0} and {n1} overlap: [{lo0}, {hi0}) and [{lo1}, {hi1})"
    bases = sorted(o.base for o in case.ops)
    assert all(b - a >= fl.SLOT for a, b in zip(bases, bases[1:]))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_narrowing_of_a_far_element_lands_in_a_compared_window(case):
    for o in case.ops:
        wins = o.windows()
        nb = o.n * o.esize
        for off in o.offs:
            for kind in fl.NARROWINGS:
                lo = fl.narrow(off, o.esize, kind)
                assert any(w0 + fl.MARGIN <= lo and lo + nb <= w1 - fl.MARGIN for w0, w1 in wins), (o.name, off, kind)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_twin_keeps_alignment_and_leading_dimension_mod_8(case):
    """The launcher must pick the same kernel for the twin: every row pointer keeps its alignment (up to 128 bytes) and every
    leading dimension its residue mod 8."""
    for o in case.ops:
        for a, b in zip(o.offs, o.twin):
            assert (a * o.esize) % 128 == (b * o.esize) % 128, (o.name, a, b)
        if "ld" in o.meta:
            assert o.meta["ld"] % 8 == o.meta["ld_twin"] % 8
        assert max(o.twin) * o.esize < 1 << 28                 # the twin is small


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_gpu_assertions_reject_every_narrowing(case):
    """The model launch with the addresses of one operand narrowed, for every operand and every narrowing that changes one of
    its offsets: assertion 1 (far output == twin output, bit for bit) or assertion 3 (nothing outside the expected outputs
    changed) must fail.  The same launch without a narrowing passes both."""
    assert fl.verdict(case) == set()
    tried = 0
    for o in case.ops:
        for kind in fl.NARROWINGS:
            if all(fl.narrow(off, o.esize, kind) == off * o.esize for off in o.offs):
                continue
            tried += 1
            failed = fl.verdict(case, o.name, kind)
            assert failed, f"{o.name} narrowed as {kind} passes assertions 1 and 3"
            if o.role != "in":
                assert failed == {1, 3}, f"{o.name} ({o.role}) narrowed as {kind}: a misplaced write must fail both, got {failed}"
    assert tried >= 4

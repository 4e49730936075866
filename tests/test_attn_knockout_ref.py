"""CPU: the reference module of the attention-knockout kernel (tests/attn_knockout_ref.py) is itself checked.  An f32 emulation of
the kernel's stream order stays inside the decode bound on every form and every kind of data the GPU test launches, and each
mutant reference — one blocked key admitted, one key too many dropped, ids >= 32 aliased, a neighbour's mask, the row lists
swapped — is rejected on every form by the assertions tests/test_gpu_attn_knockout.py uses (the count probe's and the bound on
random data), so a kernel that made one of those mistakes could not pass there."""
import pytest
import torch

import attn_knockout_ref as kr
from oracle import attention as oa


@pytest.fixture(scope="module")
def layout():
    seg = kr.make_seg()
    row_seq, row_q = kr.row_list(len(kr.LENS))
    return seg, row_seq, row_q


def _case(kind, form, layout):
    seg, row_seq, row_q = layout
    D, H, _ = form
    q, kc, vc = kr.data(kind, form)
    return kr.place_q(q, row_seq, row_q), kc, vc, kr.blocked_sets(seg, kr.LENS, row_seq, H)


def test_layout_has_what_the_cases_need(layout):
    seg, row_seq, row_q = layout
    lens = list(kr.LENS)
    ids = {int(x) for b, L in enumerate(lens) for x in seg[b, :L].tolist()}
    assert kr.UNUSED_ID not in ids and any(i >= 32 for i in ids) and any(i < 32 for i in ids) and kr.IGNORE in ids
    for b, L in enumerate(lens):        # a run boundary at 32, 33, 64 and 65 wherever the row reaches past it
        assert bool((seg[b, L:] == 0xFF).all())
        for c in (32, 33, 64, 65):
            if L > c:
                assert seg[b, c] != seg[b, c - 1], (b, c)
    assert sorted(row_seq) == list(range(len(lens))) and sorted(row_q) == list(range(len(lens)))
    for H in (3, 4, 8, 16):
        bl = kr.blocked_sets(seg, lens, row_seq, H)
        assert bool((bl == 0).any()) and bool((bl != 0).any()) and bool((bl >= 2 ** 31).any())
        assert bool((kr.as_u32_bits(bl).long() & 0xFFFFFFFF == bl).all())
        assert len({tuple(r) for r in bl.tolist()}) > len(lens) // 2          # ragged: the entries' sets differ


@pytest.mark.parametrize("form", kr.FORMS, ids=kr.form_id)
def test_emulation_stays_inside_the_decode_bound(form, layout):
    seg, row_seq, row_q = layout
    D, H, _ = form
    scale = D ** -0.5
    for kind in ("normal", "offset", "count", "peak"):
        qb, kc, vc, bl = _case(kind, form, layout)
        if kind == "peak":
            bl, n_blocked = kr.peak_blocked(seg, kr.LENS, row_seq, kr.unmasked_reference(qb, kc, vc, kr.LENS, row_seq, row_q, form, scale))
            assert n_blocked > len(row_seq) * H // 2
        R = kr.reference(qb, kc, vc, kr.LENS, seg, bl, row_seq, row_q, form, scale)
        got = kr.emulate_f32(qb, kc, vc, kr.LENS, seg, bl, row_seq, row_q, form, scale)
        worst = oa.assert_bound(got, R, D, oa.R_P["decode"], f"emulation {kr.form_id(form)} {kind}")
        if kind == "count":
            oa.assert_count(got, R, f"emulation {kr.form_id(form)} count")
        print(f"err/bound emulation {kr.form_id(form)} {kind}: {worst:.3f}")


@pytest.mark.parametrize("form", kr.FORMS, ids=kr.form_id)
def test_every_mutant_is_rejected(form, layout):
    seg, row_seq, row_q = layout
    D, H, _ = form
    scale = D ** -0.5
    bf = lambda R: R.ref.to(torch.bfloat16)
    cases = {kind: _case(kind, form, layout) for kind in ("count", "normal")}
    refs = {kind: kr.reference(qb, kc, vc, kr.LENS, seg, bl, row_seq, row_q, form, scale) for kind, (qb, kc, vc, bl) in cases.items()}
    # the reference's own rounding passes both assertions
    assert not bool(oa.fails_count(bf(refs["count"]), refs["count"]).any())
    assert not bool(oa.fails_bound(bf(refs["normal"]), refs["normal"], D, oa.R_P["decode"])[0].any())
    for mutant in kr.MUTANTS:
        for kind, (qb, kc, vc, bl) in cases.items():
            if mutant == "swap_rows" and kind == "count":
                qb = torch.zeros_like(qb)               # (a NaN query row would be rejected for the NaN alone)
            M = kr.reference(qb, kc, vc, kr.LENS, seg, bl, row_seq, row_q, form, scale, mutate=mutant)
            got = bf(M)
            if mutant == "swap_rows":                   # the mutant writes row row_seq[r]; the test reads row row_q[r]
                obuf = torch.full((len(row_seq), H, D), float("nan"), dtype=torch.bfloat16)
                obuf[torch.tensor(row_seq)] = got
                got = obuf[torch.tensor(row_q)]
            bad = oa.fails_count(got, refs[kind]) if kind == "count" else oa.fails_bound(got, refs[kind], D, oa.R_P["decode"])[0]
            assert bool(bad.any()), f"{kr.form_id(form)}: mutant {mutant} passes the {kind} assertion"


@pytest.mark.parametrize("form", [kr.FORMS[1], kr.FORMS[5]], ids=kr.form_id)
def test_ignoring_the_mask_fails_the_blocked_peak_probe(form, layout):
    """The probe of test (c): with the dominant key's segment blocked, the unmasked output is off by O(1) on every blocked pair."""
    seg, row_seq, row_q = layout
    D, H, _ = form
    scale = D ** -0.5
    qb, kc, vc, _ = _case("peak", form, layout)
    R0 = kr.unmasked_reference(qb, kc, vc, kr.LENS, row_seq, row_q, form, scale)
    bl, _ = kr.peak_blocked(seg, kr.LENS, row_seq, R0)
    R = kr.reference(qb, kc, vc, kr.LENS, seg, bl, row_seq, row_q, form, scale)
    bad, worst = oa.fails_bound(R0.ref.to(torch.bfloat16), R, D, oa.R_P["decode"])
    assert bool((bad == (bl != 0)).all()) and worst > 10

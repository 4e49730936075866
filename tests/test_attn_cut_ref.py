"""CPU: the reference module of the row-tile cut kernel (tests/attn_cut_ref.py) is itself checked.  An f32 emulation of the kernel's
stream order — a slot walking the keys of its TILE, skipping and zero-weighting what lies past its own row_len — stays inside the
decode bound on every form, every tiling and every kind of data the GPU test launches, and gives a slot the same bits in every
tiling; each mutant — one key past the causal bound, the tile's largest row_len for every slot, the next slot's mask, ids >= 32
aliased, an empty slot written, a head that is off written — is rejected by the assertions tests/test_gpu_attn_cut.py uses, on
every form that could show it (the two tile mutants need tiles of more than one slot: R > 1)."""
from functools import lru_cache

import pytest
import torch

import attn_cut_ref as cr
import attn_knockout_ref as kr
from oracle import attention as oa


@lru_cache(maxsize=None)
def _layout():
    return kr.make_seg(), cr.entries()


def _head_on(H):
    return [h % 3 != 1 for h in range(H)]


def test_layout_has_what_the_cases_need():
    seg, ents = _layout()
    assert {e.row_len for e in ents} >= set(kr.CUTS) and max(e.row_len for e in ents) == 320
    assert any(e.blocked == 0 for e in ents) and any(e.blocked >= 2 ** 31 for e in ents) and len({e.blocked for e in ents}) > len(ents) // 2
    rows = [e.row_q for e in ents]
    assert len(set(rows)) == len(rows) and min(rows) >= 2 and len(rows) < cr.n_rows(ents) - 4       # rows 0, 1 and more belong to nobody
    assert {kr.form_id(f): cr.tile_rows(f) for f in cr.FORMS} == {"D64-H3-kv3": 4, "D64-H4-kv4": 4, "D128-H3-kv3": 4, "D128-H4-kv4": 4,
                                                                   "D128-H4-kv2": 2, "D128-H8-kv2": 1, "D128-H14-kv2": 1, "D128-H16-kv2": 1}
    for R in (1, 2, 4):
        full, single, mixed = (cr.tables(ents, R, t) for t in ("full", "single", "mixed"))
        assert sorted(map(id, full.live())) == sorted(map(id, single.live())) == sorted(map(id, mixed.live())) == sorted(map(id, ents))
        for tb in (full, single, mixed, cr.tables(ents, R, "reversed")):
            assert len(tb.slots) == R * len(tb.tile_seq)
            for t, s in enumerate(tb.tile_seq):
                assert all(e is None or e.seq == s for e in tb.slots[t * R:(t + 1) * R])
        assert all(sum(e is not None for e in single.slots[t * R:(t + 1) * R]) == 1 for t in range(len(single.tile_seq)))
        if R > 1:
            assert any(e is None for e in full.slots)
            lens = [[e.row_len for e in mixed.slots[t * R:(t + 1) * R] if e is not None] for t in range(len(mixed.tile_seq))]
            assert any(1 in x and 319 in x for x in lens)                      # a tile mixing row_len 1 and 319
            assert {e.row_q for e in single.slots[0:R] if e} != {e.row_q for e in single.slots[R:2 * R] if e}


@pytest.mark.parametrize("form", cr.FORMS, ids=kr.form_id)
def test_emulation_stays_inside_the_decode_bound_in_every_tiling(form):
    seg, ents = _layout()
    D, H, _ = form
    R, scale = cr.tile_rows(form), D ** -0.5
    for kind in ("normal", "offset", "count"):
        qb, kc, vc = cr.data(kind, form, ents)
        by_row = {}
        for tiling in cr.TILINGS if kind == "normal" else ("full",):
            tb = cr.tables(ents, R, tiling)
            ref = cr.reference(tb, qb, kc, vc, seg, form, scale)
            got = cr.emulate_f32(tb, qb, kc, vc, seg, form, scale)
            found, worst = cr.violations(cr.write_out(tb, got, form, cr.n_rows(ents)), tb, ref, form, count=kind == "count")
            assert not found, (kind, tiling, found)
            print(f"err/bound emulation {kr.form_id(form)} {kind} {tiling}: {worst:.3f}")
            for e, v in zip(tb.live(), got.view(torch.int16)):
                assert torch.equal(by_row.setdefault(e.row_q, v), v), f"{tiling}: row {e.row_q} has other bits than in full tiles"


@pytest.mark.parametrize("form", cr.FORMS, ids=kr.form_id)
def test_every_mutant_is_rejected(form):
    seg, ents = _layout()
    D, H, _ = form
    R, scale, n = cr.tile_rows(form), D ** -0.5, cr.n_rows(ents)
    on = _head_on(H)
    bf = lambda ref: ref.ref.to(torch.bfloat16)
    for tiling in ("full", "mixed"):
        tb = cr.tables(ents, R, tiling)
        cases = {kind: cr.data(kind, form, ents) for kind in ("count", "normal")}
        refs = {kind: cr.reference(tb, *c, seg, form, scale) for kind, c in cases.items()}
        for kind in cases:           # the reference's own rounding passes
            assert not cr.violations(cr.write_out(tb, bf(refs[kind]), form, n, on), tb, refs[kind], form, on, count=kind == "count")[0]
        for mutant in cr.MUTANTS:
            if mutant in ("tile_max", "next_slot_mask") and R == 1:
                continue                                    # a tile of one slot has no neighbour to take anything from
            if mutant == "empty_written" and not any(e is None for e in tb.slots):
                continue                                    # (R == 1: there are no empty slots)
            for kind, c in cases.items():
                values = bf(cr.reference(tb, *c, seg, form, scale, mutate=mutant if mutant in ("len_plus1", "tile_max", "next_slot_mask", "mod32") else None))
                out = cr.write_out(tb, values, form, n, on, mutate=mutant if mutant in ("empty_written", "off_head_written") else None)
                found, _ = cr.violations(out, tb, refs[kind], form, on, count=kind == "count")
                assert found, f"{kr.form_id(form)} {tiling}: mutant {mutant} passes the {kind} assertions"


@pytest.mark.parametrize("form", [cr.FORMS[1], cr.FORMS[4]], ids=kr.form_id)
def test_ignoring_the_mask_fails_the_blocked_peak_probe(form):
    seg, ents = _layout()
    D, H, _ = form
    R, scale = cr.tile_rows(form), D ** -0.5
    qb, kc, vc = cr.data("peak", form, ents)
    zero = [cr.Entry(e.seq, e.row_len, 0, e.row_q) for e in ents]
    R0 = cr.reference(cr.tables(zero, 1), qb, kc, vc, seg, form, scale)
    peak, n_blocked = cr.peak_blocked(ents, seg, R0)
    assert n_blocked > len(ents) // 3
    tb = cr.tables(peak, R)
    ref = cr.reference(tb, qb, kc, vc, seg, form, scale)
    unmasked = cr.reference(cr.tables(zero, R), qb, kc, vc, seg, form, scale)
    found, worst = cr.violations(cr.write_out(tb, unmasked.ref.to(torch.bfloat16), form, cr.n_rows(ents)), tb, ref, form)
    assert found and worst > 10

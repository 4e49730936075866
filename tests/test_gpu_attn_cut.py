"""`-m gpu`: the row-tile cut kernel.  icl_attn_cut_rows_bf16 against the float64 reference of tests/attn_cut_ref.py with the derived
decode bound of tests/test_gpu_attention_exact.py (n and S over the visible keys; tests/test_attn_cut_ref.py shows on the CPU that it
admits an f32 emulation of the stream order and that the assertions here reject six one-mistake mutants).

Every launch works on the knockout's 22 cache sequences (1 .. 320 keys, max_len 320, NaN in the cache rows and 0xFF in the segment
bytes past each length); the listed rows are queries at every row_len of attn_knockout_ref.CUTS (1, 2, 3, 15, 16, 17, ... 319, and
the sequence's own length) over seven of those sequences, each in a row of its own of a Q buffer that is a column slice of a wider
one; O is pre-filled with a sentinel bit pattern, and rows 0, 1 and every fifth after them belong to no slot.  Tilings: full tiles
(R consecutive rows of a sequence, the tail padded with empty slots), every row alone in a tile (in slot index mod R), tiles mixing
row_len 1 and 319, the reversed tile order, and enough copies of the full tiling for more than 1024 workgroups.  One instantiation
per form — attn_decode_kernel<D, 4, false, false, 8, G, true, R> with R = 4 (G = 1), 2 (G = 2), 1 (G = 4, 7, 8) — so a slot's bits
must not depend on any of that.

Measured on MI355X: see README.md ("Attention cuts").
"""
from functools import lru_cache

import pytest
import torch

import attn_cut_ref as cr
import attn_knockout_ref as kr
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)
from oracle import attention as oa

pytestmark = pytest.mark.gpu

FORMS = [pytest.param(f, id=kr.form_id(f)) for f in cr.FORMS]


@lru_cache(maxsize=None)
def _layout():
    return kr.make_seg(), cr.entries()


@lru_cache(maxsize=None)
def _data(kind, form):
    return cr.data(kind, form, _layout()[1])


@lru_cache(maxsize=None)
def _ref(kind, form):
    """The float64 reference of the full tiling, one row per entry: computed once per (data, form) and left unchanged."""
    seg, ents = _layout()
    return cr.reference(cr.tables(ents, 1), *_data(kind, form), seg, form, form[0] ** -0.5)


def _ref_for(tb, kind, form):
    """``_ref``'s rows in the order of a table's live slots."""
    _, ents = _layout()
    at = {e.row_q: i for i, e in enumerate(ents)}
    return _ref(kind, form).rows(torch.tensor([at[e.row_q] for e in tb.live()]))


def _launch(B, form, tb, qbuf, kc, vc, *, seg=None, head_on=None, copies=1, max_len=None):
    """One launch on device copies: ``copies`` times the table's tiles, copy c reading and writing rows c * n .. of Q / O.  Returns
    the O buffer on the CPU as int16 [copies, n, H, D], the sentinel where nothing was written; asserts that nothing outside
    O's columns was touched."""
    D, H, Hkv = form
    hd, n = H * D, qbuf.shape[0]
    seg = _layout()[0] if seg is None else seg
    assert B.attn_cut_tile_rows(H, D, Hkv) == tb.R == cr.tile_rows(form)
    qw = torch.full((n * copies, hd + 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    qw[:, 32:32 + hd] = qbuf.to(DEV).repeat(copies, 1)
    ow = torch.full((n * copies, hd + 24), 0, dtype=torch.int16, device=DEV).fill_(cr.SENTINEL).view(torch.bfloat16)
    out = ow[:, 8:8 + hd]
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    row_q = [r if r < 0 else r + c * n for c in range(copies) for r in tb.row_q]
    assert all(r < n * copies for r in row_q) and all(0 <= s < kc.shape[0] for s in tb.tile_seq)
    assert all(0 <= L <= kc.shape[2] for L in tb.row_len)
    B.attn_cut_rows(qw[:, 32:32 + hd], kc.to(DEV), vc.to(DEV), out, seg.to(DEV), i32(tb.tile_seq * copies), i32(row_q),
                    i32(tb.row_len * copies), i32(cr.as_i32(tb.blocked) * copies), H, D, max_len or kc.shape[2], D ** -0.5, tile_rows=tb.R,
                    n_kv_heads=Hkv, head_on=None if head_on is None else torch.tensor(head_on, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    raw = ow.view(torch.int16)
    assert bool((raw[:, :8] == cr.SENTINEL).all()) and bool((raw[:, 8 + hd:] == cr.SENTINEL).all()), "wrote outside O's columns"
    return out.cpu().view(torch.int16).reshape(copies, n, H, D)


def _check(out, tb, kind, form, what, head_on=None):
    found, worst = cr.violations(out, tb, _ref_for(tb, kind, form), form, head_on, count=kind == "count")
    assert not found, f"{what}: {found}"
    return worst


@pytest.mark.parametrize("form", FORMS)
def test_bound(B, form):
    """Random and offset data, ragged masks, in full tiles, one live slot per tile and tiles mixing row_len 1 and 319: the decode
    bound, n and S over the visible keys; rows no slot lists keep the sentinel."""
    _, ents = _layout()
    for kind in ("normal", "offset"):
        for tiling in ("full", "single", "mixed"):
            tb = cr.tables(ents, cr.tile_rows(form), tiling)
            worst = _check(_launch(B, form, tb, *_data(kind, form))[0], tb, kind, form, f"attn_cut_rows {kr.form_id(form)} {kind} {tiling}")
            print(f"err/bound attn_cut_rows {kr.form_id(form)} {kind} {tiling}: {worst:.3f}")


@pytest.mark.parametrize("form", FORMS)
def test_count_probe(B, form):
    """q = 0, one-hot V rows: every column is (visible keys feeding it) / (visible keys); one key off moves it."""
    _, ents = _layout()
    for tiling in ("full", "mixed"):
        tb = cr.tables(ents, cr.tile_rows(form), tiling)
        _check(_launch(B, form, tb, *_data("count", form))[0], tb, "count", form, f"attn_cut_rows {kr.form_id(form)} count probe {tiling}")


@pytest.mark.parametrize("form", FORMS)
def test_blocked_peak_probe(B, form):
    """The segment of each entry's heaviest key is blocked: the output is the reference's that lacks it."""
    seg, ents = _layout()
    D = form[0]
    qb, kc, vc = _data("peak", form)
    zero = [cr.Entry(e.seq, e.row_len, 0, e.row_q) for e in ents]
    peak, n_blocked = cr.peak_blocked(ents, seg, cr.reference(cr.tables(zero, 1), qb, kc, vc, seg, form, D ** -0.5))
    assert n_blocked > len(ents) // 3
    tb = cr.tables(peak, cr.tile_rows(form))
    found, worst = cr.violations(_launch(B, form, tb, qb, kc, vc)[0], tb, cr.reference(tb, qb, kc, vc, seg, form, D ** -0.5), form)
    assert not found, found
    print(f"err/bound attn_cut_rows {kr.form_id(form)} blocked peak: {worst:.3f}")


@pytest.mark.parametrize("form", FORMS)
def test_heads_that_are_off_and_unlisted_rows_keep_the_sentinel(B, form):
    """With a head switch the heads that are off keep the sentinel in every row and the heads that are on the bits they have
    without a switch; with every head of a K/V group off the group's workgroups write nothing."""
    _, ents = _layout()
    D, H, Hkv = form
    tb = cr.tables(ents, cr.tile_rows(form))
    full = _launch(B, form, tb, *_data("normal", form))[0]
    for on in ([h % 3 != 1 for h in range(H)], [h >= H // Hkv for h in range(H)]):       # ragged; the whole first K/V group off
        out = _launch(B, form, tb, *_data("normal", form), head_on=on)[0]
        _check(out, tb, "normal", form, f"attn_cut_rows {kr.form_id(form)} head_on {on}", head_on=on)
        assert torch.equal(out[:, torch.tensor(on)], full[:, torch.tensor(on)])


@pytest.mark.parametrize("form", FORMS)
def test_batch_invariance(B, form):
    """A slot's bits are the same in full tiles, alone in a tile in every slot position, next to other companions (row_len 1 next
    to 319), in the reversed tile and slot order, and among more than 1024 workgroups."""
    _, ents = _layout()
    D, H, Hkv = form
    R = cr.tile_rows(form)
    d = _data("normal", form)
    full = _launch(B, form, cr.tables(ents, R), *d)[0]
    for tiling in ("single", "mixed", "reversed"):
        assert torch.equal(_launch(B, form, cr.tables(ents, R, tiling), *d)[0], full), f"{tiling} tiles give other bits"
    for shift in range(1, R):                                 # alone, in every other slot position
        tb = cr.tables(ents[shift:] + ents[:shift], R, "single")
        assert torch.equal(_launch(B, form, tb, *d)[0], full), f"alone in slot + {shift}: other bits"
    tb = cr.tables(ents, R)
    copies = 1024 // (len(tb.tile_seq) * Hkv) + 1
    assert len(tb.tile_seq) * Hkv <= 1024 < copies * len(tb.tile_seq) * Hkv <= 65535
    many = _launch(B, form, tb, *d, copies=copies)
    for c in range(copies):
        assert torch.equal(many[c], full), f"copy {c} of {copies} (more than 1024 workgroups) gives other bits"


def test_no_visible_key_writes_zeros(B):
    """A live slot whose mask leaves no key writes zeros; its neighbours in the tile are computed."""
    form = (128, 4, 4)
    D, H, Hkv = form
    lens = [5, 9]
    _, kc, vc = kr.data("normal", form, lens=lens, max_len=16)
    seg = torch.full((2, 16), 0xFF, dtype=torch.uint8)
    seg[0, :5], seg[1, :9] = 3, torch.tensor([0, 0, 1, 1, 1, 2, 2, 40, 40], dtype=torch.uint8)
    ents = [cr.Entry(0, 5, 8, 2), cr.Entry(0, 4, 0, 3), cr.Entry(1, 2, 1, 4), cr.Entry(1, 9, 3, 5), cr.Entry(1, 5, 3, 6)]
    qb = torch.full((8, H * D), float("nan"), dtype=torch.bfloat16)
    qb[2:7] = oa.random_data([5], H, D, seed=5)[0]
    tb = cr.tables(ents, 4)
    out = _launch(B, form, tb, qb, kc, vc, seg=seg)[0]
    assert bool((out[2] == 0).all()) and bool((out[4] == 0).all()) and bool((out[6] == 0).all())
    ref = cr.reference(tb, qb, kc, vc, seg, form, D ** -0.5)
    assert ref.n[:, 0].tolist() == [0, 4, 0, 4, 0]
    found, _ = cr.violations(out, tb, ref, form)
    assert not found, found


def test_binding_refuses_what_the_entry_point_refuses(B):
    D, H = 128, 4
    _, kc, vc = kr.data("normal", (D, H, H), lens=[5, 9], max_len=16)
    seg = torch.zeros(2, 16, dtype=torch.uint8)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=DEV)
    base = dict(q=z(8, H * D), kc=kc.to(DEV), vc=vc.to(DEV), out=z(8, H * D), seg=seg.to(DEV), tile_seq=i32([0, 1]),
                row_q=i32([0, 1, -1, -1, 2, 3, 4, -1]), row_len=i32([5, 3, 0, 0, 9, 1, 2, 0]), blocked=i32([0] * 8), H=H, D=D, max_len=16,
                scale=D ** -0.5, R=4, Hkv=0, head_on=None)

    def call(**kw):
        a = dict(base, **kw)
        B.attn_cut_rows(a["q"], a["kc"], a["vc"], a["out"], a["seg"], a["tile_seq"], a["row_q"], a["row_len"], a["blocked"], a["H"], a["D"],
                        a["max_len"], a["scale"], tile_rows=a["R"], n_kv_heads=a["Hkv"], head_on=a["head_on"])
    call()                                                                       # the valid call
    call(head_on=torch.tensor([1, 0, 1, 1], dtype=torch.uint8, device=DEV))
    assert [B.attn_cut_tile_rows(H, D, kv) for kv in (0, 4, 2, 1)] == [4, 4, 2, 1] and B.attn_cut_tile_rows(4, 64) == 4
    for bad in ((8, 64, 4), (18, 128, 2), (4, 96, 4), (4, 128, 3)):
        with pytest.raises(B.IclError, match="icl_attn_cut_tile_rows"):
            B.attn_cut_tile_rows(*bad)
    wide = z(8, H * D + 8)
    empty = dict(tile_seq=i32([]), row_q=i32([]), row_len=i32([]), blocked=i32([]))
    two = dict(row_q=i32([0, 1, 2, 3]), row_len=i32([5, 3, 9, 1]), blocked=i32([0] * 4))          # tables built for R = 2
    refusals = {
        "n_tiles": empty,
        "tile_rows": dict(R=2, **two),
        "head_dim": dict(D=96),
        "n_kv_heads": dict(Hkv=3),
        "G at most 8": dict(H=18, Hkv=2, R=1, q=z(8, 18 * D), out=z(8, 18 * D), row_q=i32([0, 1]), row_len=i32([5, 3]), blocked=i32([0, 0])),
        "only 128": dict(D=64, H=8, Hkv=4, R=2, **two),
        "ld_seg": dict(seg=seg[:, :15].contiguous().to(DEV)),
        "misaligned": dict(q=wide[:, 4:4 + H * D]),
        "ldq": dict(q=z(8, H * D - 8)),
        "ldo": dict(out=z(8, H * D - 8)),
        "scale": dict(scale=float("inf")),
    }
    for word, kw in refusals.items():
        with pytest.raises(B.IclError, match="icl_attn_cut_rows_bf16.*" + word):
            call(**kw)
    torch.cuda.synchronize()

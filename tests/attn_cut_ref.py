"""The float64 reference of icl_attn_cut_rows_bf16 (attention cuts between prompt segments), the tile tables of
tests/test_gpu_attn_cut.py, deliberately wrong executions (mutants) and an f32 emulation of the kernel's stream order.  Plain torch /
numpy on the CPU; tests/test_attn_cut_ref.py shows without a GPU that the decode bound admits the emulation and that the assertions
of the GPU test reject every mutant on every form that could show it.

Definition (include/icl_hip.h): tile t works on cache sequence tile_seq[t]; its slot e = t * R + r reads the query at row row_q[e]
(< 0: an empty slot) and writes that row of O; key j counts for slot e iff j < row_len[e] and not (seg_j < 32 and bit seg_j of
blocked[e]).  A head that is off (head_on) is not written.

The reference is oracle.attention._group_ref, one call per (live slot, query head), ``visible = (j < row_len) & ~blocked(seg[j])``,
so the bound is the decode bound of tests/test_gpu_attention_exact.py (oracle.attention.err_bound, r_P = 0) with n and S taken over
the visible keys.  No new tolerance.

Shapes are the knockout's (tests/attn_knockout_ref.py): its FORMS, its 22 cache sequences of 1 .. 320 keys at max_len 320 with NaN
in the cache rows past each length, its segment layout.  The listed rows: for each of SEQS (cache sequences of 3 .. 320 keys) a
query at every row_len of attn_knockout_ref.CUTS below the sequence's length, and one at the length itself.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

import attn_knockout_ref as kr
from oracle import attention as oa

LENS = kr.LENS
MAX_LEN = kr.MAX_LEN
FORMS = kr.FORMS
SEQ_LENS = (3, 17, 33, 65, 129, 257, 320)                  # the cache sequences that carry listed rows
SEQS = tuple(LENS.index(L) for L in SEQ_LENS)
SENTINEL = 0x7FA5                                          # a NaN bit pattern no kernel writes (int16 view of bf16)
MUTANTS = ("len_plus1", "tile_max", "next_slot_mask", "mod32", "empty_written", "off_head_written")
TILINGS = ("full", "single", "mixed", "reversed")


def tile_rows(form):
    """R of a form, as the host asks the library for it (icl_attn_cut_tile_rows, a host query that needs no GPU): 4 multi-head, 2
    at G = 2, 1 from G = 3 on."""
    from icl_speech_text_llm_amd.runtime import binding
    D, H, Hkv = form
    return binding.attn_cut_tile_rows(H, D, Hkv)


@dataclass
class Entry:
    seq: int          # cache sequence
    row_len: int      # the keys the query may see
    blocked: int      # u32 bit set
    row_q: int        # row of Q / O


def entries(seed=kr.SEED) -> List[Entry]:
    """The listed rows, ascending by (sequence, row_len).  Row r of Q / O belongs to entry ``perm[r]``; rows 0 and 1 and every
    fifth row after them belong to nobody (they must keep the sentinel).  Masks: per entry a random subset of the ids below 32
    among its visible keys, plus kr.UNUSED_ID and the bits that ids >= 32 alias to; every fourth entry keeps mask 0; a set that
    would leave no key gives up the id of the entry's last key."""
    seg = kr.make_seg()
    g = np.random.default_rng(seed + 11)
    out = []
    for s in SEQS:
        L = LENS[s]
        for rl in [c for c in kr.CUTS if c < L] + [L]:
            m = 0
            if len(out) % 4 != 3:
                present = sorted({int(x) for x in seg[s, :rl].tolist() if x < 32})
                for i in present + [kr.UNUSED_ID, 8, 1, 31]:
                    if g.random() < 0.5:
                        m |= 1 << i
                if not bool(kr.visible_of(seg[s], rl, m).any()):
                    m &= ~(1 << int(seg[s, rl - 1]))
            assert bool(kr.visible_of(seg[s], rl, m).any())
            out.append(Entry(s, rl, m, -1))
    free = [r for r in range(2 + len(out) * 5 // 4 + 2) if r >= 2 and (r - 2) % 5 != 4]
    perm = np.random.default_rng(seed + 12).permutation(len(out))
    for e, k in zip(out, perm):
        e.row_q = free[int(k)]
    return out


def n_rows(ents) -> int:
    return max(e.row_q for e in ents) + 3


@dataclass
class Tables:
    R: int
    tile_seq: List[int]
    slots: List[Optional[Entry]]          # n_tiles * R, None: an empty slot

    @property
    def row_q(self):
        return [-1 if e is None else e.row_q for e in self.slots]

    @property
    def row_len(self):
        return [0 if e is None else e.row_len for e in self.slots]

    @property
    def blocked(self):
        return [0 if e is None else e.blocked for e in self.slots]

    def live(self):
        return [e for e in self.slots if e is not None]


def tables(ents, R, tiling="full") -> Tables:
    """full: R consecutive entries of one sequence per tile, the tail of a sequence's last tile empty; single: every entry alone
    in a tile, in slot (its index) mod R; mixed: a sequence's entries taken from both ends in turn, so that a tile holds its
    shortest next to its longest row_len (1 next to 319); reversed: the tiles of full in the reversed order, the slots of each
    tile reversed too."""
    assert tiling in TILINGS
    tile_seq, slots = [], []
    if tiling == "single":
        for i, e in enumerate(ents):
            tile_seq.append(e.seq)
            slots += [e if r == i % R else None for r in range(R)]
        return Tables(R, tile_seq, slots)
    for s in sorted({e.seq for e in ents}):
        own = [e for e in ents if e.seq == s]
        if tiling == "mixed":
            rest = own[:-1]                           # (the entry at the sequence's own length goes last)
            own = [rest[i // 2] if i % 2 == 0 else rest[-1 - i // 2] for i in range(len(rest))] + own[-1:]
        for i in range(0, len(own), R):
            part = own[i:i + R]
            tile_seq.append(s)
            slots += part + [None] * (R - len(part))
    if tiling == "reversed":
        tile_seq = tile_seq[::-1]
        slots = slots[::-1]
    return Tables(R, tile_seq, slots)


def data(kind, form, ents, seed=kr.SEED):
    """(Q buffer [n_rows, H * D]: entry e's query in row e.row_q, NaN elsewhere; kc, vc [22, Hkv, MAX_LEN, D]) bf16 on the CPU.
    The caches are the knockout's of the same kind; the queries are random (count: zero; peak: the sequence's peak query for
    every entry of the sequence)."""
    D, H, Hkv = form
    qs, kc, vc = kr.data(kind, form)
    if kind == "count":
        q = torch.zeros(len(ents), H * D, dtype=torch.bfloat16)
    elif kind == "peak":
        q = qs[torch.tensor([e.seq for e in ents])]
    else:
        q = oa.random_data([len(ents)], H, D, seed=seed + 5, offset=kind == "offset")[0]
    buf = torch.full((n_rows(ents), H * D), float("nan"), dtype=torch.bfloat16)
    buf[torch.tensor([e.row_q for e in ents])] = q
    return buf, kc, vc


def _entry_ref(e: Entry, qbuf, kc, vc, seg, form, scale, row_len=None, blocked=None, mod32=False):
    rl = e.row_len if row_len is None else row_len
    vis = kr.visible_of(seg[e.seq], rl, e.blocked if blocked is None else blocked, mod32=mod32)
    return kr.entry_ref(qbuf[e.row_q], kc[e.seq], vc[e.seq], [vis] * form[1], form, scale, e.seq)


def reference(tb: Tables, qbuf, kc, vc, seg, form, scale, mutate=None) -> oa.Ref:
    """One Ref row per live slot, in table order: what row row_q of O must hold.  ``mutate``: len_plus1 (one key past the causal
    bound counts, where the sequence has one), tile_max (the tile's largest row_len for every slot), next_slot_mask (the mask
    of the tile's next live slot, cyclically), mod32 (an id >= 32 is treated as id mod 32)."""
    rows = []
    for t in range(len(tb.tile_seq)):
        live = [e for e in tb.slots[t * tb.R:(t + 1) * tb.R] if e is not None]
        for i, e in enumerate(live):
            rl, bl = None, None
            if mutate == "len_plus1" and e.row_len < LENS[e.seq]:
                rl = e.row_len + 1
            if mutate == "tile_max":
                rl = max(x.row_len for x in live)
            if mutate == "next_slot_mask":
                bl = live[(i + 1) % len(live)].blocked
            rows.append(_entry_ref(e, qbuf, kc, vc, seg, form, scale, rl, bl, mod32=mutate == "mod32"))
    return oa.Ref.cat(rows)


def write_out(tb: Tables, values, form, n, head_on=None, mutate=None):
    """The O buffer [n, H, D] an execution leaves, as int16 bit patterns: the sentinel everywhere, ``values`` (bf16 [live slots,
    H, D], table order) in the rows of the live slots, heads that are off left alone.  ``mutate``: empty_written (an empty slot
    is written to the row its clamped index names, row 0), off_head_written (a head that is off is written)."""
    D, H, _ = form
    out = torch.full((n, H, D), SENTINEL, dtype=torch.int16)
    on = torch.ones(H, dtype=torch.bool) if head_on is None or mutate == "off_head_written" else torch.as_tensor(head_on).bool()
    for v, e in zip(values.view(torch.int16), tb.live()):
        out[e.row_q, on] = v[on]
    if mutate == "empty_written" and any(e is None for e in tb.slots):
        out[0, on] = 0
    return out


def violations(out, tb: Tables, R: oa.Ref, form, head_on=None, count=False):
    """What the GPU test asserts of an O buffer (int16 [n, H, D]), as a list of findings (empty: it passes): rows no live slot
    lists and heads that are off keep the sentinel; the heads that are on of every listed row are inside the decode bound of the
    reference (``count``: within one bf16 ulp of the count probe's)."""
    D, H, _ = form
    on = torch.ones(H, dtype=torch.bool) if head_on is None else torch.as_tensor(head_on).bool()
    rows = torch.tensor([e.row_q for e in tb.live()])
    listed = torch.zeros(out.shape[0], dtype=torch.bool)
    listed[rows] = True
    found = []
    if not bool((out[~listed] == SENTINEL).all()):
        found.append("a row no slot lists was written")
    if not bool((out[:, ~on] == SENTINEL).all()):
        found.append("a head that is off was written")
    got = out[rows].view(torch.bfloat16)
    sub = lambda x: x[:, on] if x.dim() > 1 else x
    Ron = oa.Ref(*[sub(getattr(R, f)) for f in ("ref", "A", "vt", "S", "n", "pmax", "tgt", "vdom", "seq", "pos")])
    if count:
        bad = oa.fails_count(got[:, on], Ron)
        worst = float("nan")
    else:
        bad, worst = oa.fails_bound(got[:, on], Ron, D, oa.R_P["decode"])
    if bool(bad.any()):
        found.append(f"err/bound {worst:.3g} at {oa.describe(Ron, bad)}")
    return found, worst


def peak_blocked(ents, seg, R0: oa.Ref):
    """Masks for the blocked-peak probe: per entry the segment of the heaviest key of head 0 (``R0``: the reference with every
    mask 0, entries in order), 0 where that id is >= 32 or where the segment is all the entry can see.  Returns (entries with
    those masks, how many are non-zero)."""
    out, n = [], 0
    for i, e in enumerate(ents):
        g = int(seg[e.seq, int(R0.tgt[i, 0])])
        m = 1 << g if g < 32 and bool(kr.visible_of(seg[e.seq], e.row_len, 1 << g).any()) else 0
        n += m != 0
        out.append(Entry(e.seq, e.row_len, m, e.row_q))
    return out, n


def as_i32(bits):
    """u32 bit sets as the int32 values the binding takes."""
    return [b - (1 << 32) if b >= (1 << 31) else b for b in bits]


# ------------------------------------------------------------------------------------------------------------------
# an f32 emulation of the kernel's stream order
# ------------------------------------------------------------------------------------------------------------------
def emulate_f32(tb: Tables, qbuf, kc, vc, seg, form, scale):
    """attn_decode_kernel<.., MASK, R> in numpy float32, bf16 [live slots, H, D] in table order: the stream order of the knockout's
    kernel (``attn_knockout_ref.emulate_head_f32``), every slot walking the keys 0 .. the TILE's largest row_len - 1 — a key at or
    past the slot's own row_len or under its mask has weight 0, and a group of four wholly past its row_len is not entered."""
    D, H, Hkv = form
    G, NS = H // Hkv, 4 * (64 // (D // 8))
    outs = []
    for t in range(len(tb.tile_seq)):
        live = [e for e in tb.slots[t * tb.R:(t + 1) * tb.R] if e is not None]
        Lt = max(e.row_len for e in live)
        for e in live:
            ok = kr.visible_of(seg[e.seq], e.row_len, e.blocked)
            outs.append(np.stack([kr.emulate_head_f32(qbuf[e.row_q].view(H, D)[h], kc[e.seq, h // G], vc[e.seq, h // G], ok, Lt, NS, scale)
                                  for h in range(H)]))
    return kr._bf16_round(np.stack(outs))

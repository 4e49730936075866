"""The float64 reference of icl_attn_decode_masked_bf16 (attention knockout), the segment layouts, blocked sets and row lists of
tests/test_gpu_attn_knockout.py, deliberately wrong references (mutants) and an f32 emulation of the kernel's stream order.  Plain
torch / numpy on the CPU; tests/test_attn_knockout_ref.py shows without a GPU that the decode bound admits the emulation and that
the assertions of the GPU test reject every mutant on every form.

Definition (include/icl_hip.h): list entry r reads the query at row row_q[r], attends over cache sequence row_seq[r] and writes row
row_q[r]; key j counts for query head h iff j < lens[row_seq[r]] and not (seg_j < 32 and bit seg_j of blocked[r][h]).

The reference is oracle.attention._group_ref, one call per (list entry, query head) with that head's own ``visible`` row, so the
bound is the one of tests/test_gpu_attention_exact.py (oracle.attention.err_bound, r_P = 0 for decode) with n and S taken over
the visible keys: a masked key enters no sum, so it owes no error term.  No new tolerance.

Every launch covers oracle.attention.DECODE_LENS (22 cache rows of 1 .. 320 keys) at max_len 320, NaN in the cache rows and 0xFF in
the segment bytes past each length.  Every listed (row, head) keeps at least one visible key: ``blocked_sets`` asserts it, so no
case is ever skipped.
"""
from __future__ import annotations

from dataclasses import fields

import numpy as np
import torch

from oracle import attention as oa

LENS = tuple(oa.DECODE_LENS)
MAX_LEN = 320
SEED = 7331
IGNORE = 255
UNUSED_ID = 5                   # a segment id below 32 that no layout uses: blocking it changes nothing
# run ids in the order a row's runs take them: most below 32, some at or above (40 = 8 mod 32, 200 = 8 mod 32, 33 = 1 mod 32, 255)
RUN_IDS = (0, 3, 40, 1, 31, 200, 2, 7, IGNORE, 4, 6, 33, 9, 30, 8)
# run boundaries: at and next to the stream strides (4 * KPW keys = 16 at head_dim 128, 32 at 64) and their multiples
CUTS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 96, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 319)
MUTANTS = ("admit_one", "drop_after", "mod32", "head_plus1", "entry_plus1", "swap_rows")

# (head_dim, query heads, K/V heads): multi-head at 64 / 128 and H = 3 / 4, grouped at 128 with G = 2, 4, 7, 8
FORMS = [(64, 3, 3), (64, 4, 4), (128, 3, 3), (128, 4, 4), (128, 4, 2), (128, 8, 2), (128, 14, 2), (128, 16, 2)]


def form_id(form):
    D, H, Hkv = form
    return f"D{D}-H{H}-kv{Hkv}"


def many_reps(Hkv):
    """Copies of the 22-entry list that put more than 1024 workgroups (the launcher's few / many switch) into one launch."""
    return 1024 // (len(LENS) * Hkv) + 1


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
def make_seg(lens=LENS, max_len=MAX_LEN, seed=SEED):
    """uint8 [len(lens), max_len]: every row cut into ragged runs at a random subset of CUTS (rows of >= 34 keys always cut at 32
    and 33, rows of >= 66 at 64 and 65: one-key runs on both sides of a stride), the runs taking RUN_IDS in turn from a row-
    dependent start.  UNUSED_ID appears nowhere.  Bytes at or past the length are 0xFF."""
    g = np.random.default_rng(seed)
    seg = np.full((len(lens), max_len), 0xFF, dtype=np.uint8)
    for b, L in enumerate(lens):
        cuts = {c for c in CUTS if c < L and g.random() < 0.45}
        cuts |= {c for c in (31, 32, 33) if L >= 34} | {c for c in (63, 64, 65) if L >= 66}
        edges = [0] + sorted(cuts) + [L]
        for i, (a, e) in enumerate(zip(edges[:-1], edges[1:])):
            seg[b, a:e] = RUN_IDS[(i + 2 * b) % len(RUN_IDS)]
    assert not bool((seg == UNUSED_ID).any())
    return torch.from_numpy(seg)


def visible_of(seg_row, L, mask, *, mod32=False):
    """bool [L]: the keys of one (list entry, head).  ``mod32`` (a mutant): an id >= 32 is treated as id mod 32."""
    ids = seg_row[:L].long()
    bit = (torch.full_like(ids, int(mask)) >> (ids & 31)) & 1
    if mod32:
        return bit == 0
    return ~((ids < 32) & (bit == 1))


def blocked_sets(seg, lens, row_seq, H, seed=SEED, zero_every=5):
    """int64 [len(row_seq), H] bit sets, ragged: per (entry, head) a random subset of the ids below 32 present in the row, plus
    UNUSED_ID and the bits 8, 1 and 31 that ids 40 / 200, 33 and 255 alias to (blocked only if such an id is its own run's id
    too).  Every ``zero_every``-th (entry, head) pair keeps mask 0.  A set that would leave no key gives up the id of the row's
    last key; asserted: every pair keeps at least one visible key."""
    g = np.random.default_rng(seed + 1)
    out = torch.zeros(len(row_seq), H, dtype=torch.int64)
    for r, s in enumerate(row_seq):
        L = int(lens[s])
        present = sorted({int(x) for x in seg[s, :L].tolist() if x < 32})
        for h in range(H):
            if (r * H + h) % zero_every == 0:
                continue
            m = 0
            for i in present + [UNUSED_ID, 8, 1, 31]:
                if g.random() < 0.5:
                    m |= 1 << i
            if not bool(visible_of(seg[s], L, m).any()):
                m &= ~(1 << int(seg[s, L - 1]))
            out[r, h] = m
    assert_some_key_visible(seg, lens, row_seq, out)
    return out


def assert_some_key_visible(seg, lens, row_seq, blocked):
    for r, s in enumerate(row_seq):
        for h in range(blocked.shape[1]):
            assert bool(visible_of(seg[s], int(lens[s]), int(blocked[r, h])).any()), f"entry {r} head {h}: no visible key"


def as_u32_bits(blocked):
    """The bit sets as the int32 tensor the binding takes (bit 31 set = a negative int32)."""
    b = blocked.clone()
    b[b >= 2 ** 31] -= 2 ** 32
    return b.to(torch.int32)


def row_list(n, seed=SEED):
    """(row_seq, row_q): the sequences in a shuffled order, each with its query in a row of Q / O other than its own."""
    g = torch.Generator().manual_seed(seed + 2)
    row_seq = torch.randperm(n, generator=g)
    row_q = torch.roll(row_seq, 3)
    assert not bool((row_seq == row_q).any())
    return row_seq.tolist(), row_q.tolist()


def expand_kv(x, Hkv, G, D):
    return x.view(x.shape[0], Hkv, D).repeat_interleave(G, dim=1).reshape(x.shape[0], Hkv * G * D)


def data(kind, form, lens=LENS, max_len=MAX_LEN):
    """(q [n, H * D]: sequence s's query in row s, kc, vc [n, Hkv, max_len, D]) bf16 on the CPU: the probes and random data of
    oracle/attention.py, a K/V head shared by G query heads (peak: build g of ``probe_peak`` has the same k / v for every g)."""
    D, H, Hkv = form
    G, lens = H // Hkv, list(lens)
    if kind == "count":
        _, k, v = oa.probe_count(lens, Hkv, D)
        q = torch.zeros(sum(lens), H * D, dtype=torch.bfloat16)
    elif kind == "peak":
        builds = [oa.probe_peak(lens, Hkv, D, head_offset=g) for g in range(G)]
        k, v = builds[0][1], builds[0][2]
        assert all(torch.equal(b[1], k) and torch.equal(b[2], v) for b in builds)
        q = torch.stack([b[0].view(-1, Hkv, D) for b in builds], dim=2).reshape(-1, H * D)
    else:
        q, _, _ = oa.random_data(lens, H, D, offset=kind == "offset")
        _, k, v = oa.random_data(lens, Hkv, D, seed=oa.SEED + 1, offset=kind == "offset")
    kc, vc = oa.to_cache(k, v, lens, Hkv, D, max_len)
    return oa.last_rows(q, lens).contiguous(), kc, vc


def place_q(q, row_seq, row_q):
    """The Q buffer of a list: sequence row_seq[r]'s query in row row_q[r], NaN elsewhere."""
    buf = torch.full_like(q, float("nan"))
    buf[torch.tensor(row_q)] = q[torch.tensor(row_seq)]
    return buf


# ------------------------------------------------------------------------------------------------------------------
# the reference and its mutants
# ------------------------------------------------------------------------------------------------------------------
def _cat_heads(parts):
    """Refs of one row, one head each -> one Ref row with H heads."""
    out = []
    for f in fields(oa.Ref):
        xs = [getattr(p, f.name) for p in parts]
        out.append(xs[0] if f.name in ("seq", "pos") else torch.cat(xs, dim=1))
    return oa.Ref(*out)


def entry_ref(q_row, kc_s, vc_s, visible, form, scale, seq) -> oa.Ref:
    """The fp64 reference of one listed row, a Ref row with H heads: the query ``q_row`` [H * D] over the cache of one sequence
    (``kc_s``, ``vc_s`` [Hkv, max_len, D]), head h over the keys ``visible[h]`` (bool [n keys]: the row reads keys 0 .. n - 1)."""
    D, H, Hkv = form
    G = H // Hkv
    heads = []
    for h, vis in enumerate(visible):
        n, kh = len(vis), h // G
        heads.append(oa._group_ref(q_row.view(H, 1, D)[h:h + 1], kc_s[kh:kh + 1, :n], vc_s[kh:kh + 1, :n], vis[None], scale,
                                   None, None, None, seq, [n - 1]))
    return _cat_heads(heads)


def reference(qbuf, kc, vc, lens, seg, blocked, row_seq, row_q, form, scale, mutate=None) -> oa.Ref:
    """One Ref row per list entry, in list order: what row row_q[r] of O must hold.  ``mutate``: one of MUTANTS — admit_one (the
    first blocked key of a (entry, head) counts), drop_after (the first key after a blocked run is dropped too), mod32 (an id >= 32
    is treated as id mod 32), head_plus1 / entry_plus1 (the mask of the next head / list entry, cyclically), swap_rows (row_seq
    and row_q change places: the wrong query meets the wrong sequence)."""
    assert mutate is None or mutate in MUTANTS
    D, H, Hkv = form
    rows, n_list = [], len(row_seq)
    for r in range(n_list):
        s, rq = (row_q[r], row_seq[r]) if mutate == "swap_rows" else (row_seq[r], row_q[r])
        L = int(lens[s])
        heads = []
        for h in range(H):
            m = int(blocked[(r + 1) % n_list if mutate == "entry_plus1" else r, (h + 1) % H if mutate == "head_plus1" else h])
            vis = visible_of(seg[s], L, m, mod32=mutate == "mod32").clone()
            gone = torch.nonzero(~vis)[:, 0]
            if mutate == "admit_one" and gone.numel():
                vis[gone[0]] = True
            if mutate == "drop_after" and gone.numel():
                after = [int(j) + 1 for j in gone if int(j) + 1 < L and bool(vis[int(j) + 1])]
                if after:
                    vis[after[0]] = False
            heads.append(vis)
        rows.append(entry_ref(qbuf[rq], kc[s], vc[s], heads, form, scale, s))
    return oa.Ref.cat(rows)


def unmasked_reference(qbuf, kc, vc, lens, row_seq, row_q, form, scale) -> oa.Ref:
    """The reference with every mask 0 (oracle.attention.decode_ref's rows, for grouped caches too)."""
    zero = torch.zeros(len(row_seq), form[1], dtype=torch.int64)
    seg = torch.full((len(lens), kc.shape[2]), IGNORE, dtype=torch.uint8)
    return reference(qbuf, kc, vc, lens, seg, zero, row_seq, row_q, form, scale)


def peak_blocked(seg, lens, row_seq, R0: oa.Ref):
    """[n_list, H] bit sets for the blocked-peak probe: the segment of each (entry, head)'s dominant key ``R0.tgt`` (R0: the
    unmasked reference), 0 where that id is >= 32 or where the segment is all the row has.  Returns (blocked, pairs blocked)."""
    out = torch.zeros(tuple(R0.tgt.shape), dtype=torch.int64)
    for r, s in enumerate(row_seq):
        L = int(lens[s])
        for h in range(out.shape[1]):
            g = int(seg[s, int(R0.tgt[r, h])])
            if g < 32 and bool(visible_of(seg[s], L, 1 << g).any()):
                out[r, h] = 1 << g
    assert_some_key_visible(seg, lens, row_seq, out)
    return out, int((out != 0).sum())


# ------------------------------------------------------------------------------------------------------------------
# an f32 emulation of the kernel's stream order
# ------------------------------------------------------------------------------------------------------------------
def _bf16_round(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.bfloat16)


def emulate_head_f32(qh, k, v, ok, walk, NS, scale):
    """One (listed row, query head) of attn_decode_kernel<.., MASK[, R]> in numpy float32, f32 [D]: 4 * KPW = ``NS`` streams (key j
    belongs to stream j mod NS, KPW = 64 / (D / 8)), each folding its keys in groups of four with one running-maximum update per
    group, base-2 exponentials of scores scaled by scale * log2(e); the streams merged once (zeros where no key counts).  ``qh``
    bf16 [D]; ``k``, ``v`` bf16 [>= walk, D]; ``ok`` bool [row_len]: the keys that count.  The keys 0 .. ``walk`` - 1 are walked (the
    row's own row_len, or the largest of its tile); a key at or past row_len or not ``ok`` has score -1e30 and weight 0, and a
    group of four wholly past row_len is not entered."""
    f, D, row_len = np.float32, k.shape[1], len(ok)
    T = -(-walk // (4 * NS)) * 4 * NS
    okT = np.zeros(T, dtype=bool)
    okT[:row_len] = ok.numpy()
    qv = (qh.float().numpy() * f(scale * 1.4426950408889634)).astype(f)
    kT, vT = np.zeros((T, D), dtype=f), np.zeros((T, D), dtype=f)
    kT[:walk], vT[:walk] = k[:walk].float().numpy(), v[:walk].float().numpy()
    sc = np.where(okT, (kT @ qv).astype(f), f(-1.0e30)).reshape(-1, 4, NS)                 # key = (it * 4 + i) * NS + stream
    okr, vr = okT.reshape(-1, 4, NS), vT.reshape(-1, 4, NS, D)
    m, l, o = np.full(NS, -1.0e30, dtype=f), np.zeros(NS, dtype=f), np.zeros((NS, D), dtype=f)
    for it in range(sc.shape[0]):
        go = it * 4 * NS + np.arange(NS) // (NS // 4) * (NS // 4) < row_len                 # the group's first key of the stream's wave
        m_new = np.maximum(m, sc[it].max(0))
        alpha = np.exp2(m - m_new).astype(f)
        pe = np.where(okr[it], np.exp2(sc[it] - m_new[None]).astype(f), f(0))
        l2 = (l * alpha + ((pe[0] + pe[1]) + (pe[2] + pe[3]))).astype(f)
        o2 = (o * alpha[:, None]).astype(f)
        for i in range(4):
            o2 = (o2 + pe[i][:, None] * vr[it, i]).astype(f)
        m, l, o = np.where(go, m_new, m), np.where(go, l2, l), np.where(go[:, None], o2, o)
    w = np.exp2(m - m.max()).astype(f)
    Lsum, acc = f(0), np.zeros(D, dtype=f)
    for st in range(NS):
        Lsum = f(Lsum + l[st] * w[st])
        acc = (acc + o[st] * w[st]).astype(f)
    return acc / Lsum if Lsum > 0 else np.zeros(D, dtype=f)


def emulate_f32(qbuf, kc, vc, lens, seg, blocked, row_seq, row_q, form, scale):
    """attn_decode_kernel<.., MASK> in numpy float32 (``emulate_head_f32``, every row walking its own keys): bf16 [n_list, H, D] in
    list order."""
    D, H, Hkv = form
    G, NS = H // Hkv, 4 * (64 // (D // 8))
    out = np.zeros((len(row_seq), H, D), dtype=np.float32)
    for r, (s, rq) in enumerate(zip(row_seq, row_q)):
        L = int(lens[s])
        for h in range(H):
            out[r, h] = emulate_head_f32(qbuf[rq].view(H, D)[h], kc[s, h // G], vc[s, h // G], visible_of(seg[s], L, int(blocked[r, h])),
                                         L, NS, scale)
    return _bf16_round(out)

"""What the decoder probes put into their workspace buffers, without a GPU: runtime/probes.py builds its device state with plain
torch, so on ``Workspace("cpu")`` every table can be read back.  The launch trace (tests/test_launch_trace.py) pins which buffers
are requested and what is launched on them; this file pins their CONTENT — the knockout's per-head bit sets, the segment tables,
the cuts' lists and decode-step table, the head patch's sorted pairs and permuted vectors — and how that state is re-sliced to
a prefill chunk (``rows``) and to the kept rows of ``overlong="drop"`` (``kept``).  Every expected value is written out by hand
from the definitions in the docstrings of runtime/probes.py and ``generate``; none is computed by the code under test."""
from dataclasses import replace

import pytest
import torch

BIT31 = -(1 << 31)                 # bit 31 of a u32 bit set alone, as the int32 that holds it
X = 255                            # the segment id past a prompt's end


@pytest.fixture(scope="module")
def cfg():
    """head_dim 64, four heads, two layers (launch_trace's tiny_h4): the row-tile form holds four rows."""
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    return replace(SalmonnCfg.tiny().llama, n_heads=4, n_layers=2)


def _probes(cfg, plens, max_len=8, kv="bf16", **kw):
    """(the validated arguments, the bundle on a CPU workspace, the workspace) of ``generate(**kw)`` over prompts of ``plens``."""
    from icl_speech_text_llm_amd.runtime import probes as P
    from icl_speech_text_llm_amd.runtime.engines import Workspace
    v = P.check_probes(cfg, kv, list(plens), 1, **kw)
    ws = Workspace("cpu")
    return v, v.state(ws, cfg, len(plens), max_len), ws


def _again(cfg, v, plens, max_len=8):
    """The bundle of validated arguments handed in again as the caller's (what ``overlong="drop"`` does with the kept rows')."""
    return _probes(cfg, plens, max_len, **vars(v))


def _rowlist(listed):
    return listed.seqs, listed.dev.tolist(), listed.dev.dtype


def test_a_plain_call_builds_nothing(cfg):
    v, probes, ws = _probes(cfg, (3, 2))
    assert vars(v) == dict(knockout=None, patch=None, head_patch=None, cuts=None, want_hidden=False, want_heads=False)
    assert ws.nbytes() == 0 and probes.rows(0, 2) is None and probes.decode_steps() is None and probes.graph_key() == ()
    # ... and so do probes that list nothing: empty blocked sets, an empty row list, pairs no query meets
    v, probes, ws = _probes(cfg, (3, 2), knockout=([[0, 1, 31], [0, 0]], [[], []]), patch=dict(site=0, vectors=torch.zeros(256), rows=[]),
                            head_patch=dict(heads=[(0, 0)], vectors=torch.zeros(1, 64), rows=[]),
                            cuts=dict(segments=[[0, 1, 31], [0, 0]], pairs=[(0, 1), (5, 0)]))
    assert (v.knockout, v.patch, v.head_patch, v.cuts) == (None,) * 4 and ws.nbytes() == 0 and probes.rows(0, 2) is None


def test_knockout_blocked_table_with_bit_31_and_a_head_subset(cfg):
    _, probes, ws = _probes(cfg, (3, 2), knockout=([[0, 1, 31], [0, 0]], [[31, 1], []], (0, 1), [1]))
    ko = probes.knockout
    assert ko.blocked.tolist() == [[0, -2147483646, 0, 0]] and ko.blocked.dtype == torch.int32      # bits 1 and 31, head 1 alone
    assert _rowlist(ko.listed) == ((0,), [0], torch.int32)
    assert ko.seg.tolist() == [[0, 1, 31, X, X, X, X, X], [0, 0, X, X, X, X, X, X]] and ko.seg.dtype == torch.uint8
    assert ko.layers == (0, 1) and ko.uid == ("knockout", 1, 0, 1) and ko.covers(0) and not ko.covers(1)
    assert sorted(n for n, _ in ws._bufs) == ["gen_ko_blocked", "gen_ko_rows", "gen_ko_seg"]
    assert probes.decode_steps().knockout is ko and probes.graph_key() == (("knockout", 1, 0, 1),)


def test_knockout_of_all_heads_and_its_rows(cfg):
    _, probes, _ = _probes(cfg, (3, 2, 4), knockout=dict(segments=[[0, 1, 2], [7, 7], [0, 3, 3, 40]], blocked=[[2], [], [3, 0]]))
    ko = probes.knockout
    assert ko.blocked.tolist() == [[4] * 4, [9] * 4] and _rowlist(ko.listed)[:2] == ((0, 2), [0, 2])
    assert ko.layers == (0, 2) and ko.uid == ("knockout", 2, 0, 2)
    assert ko.seg.tolist() == [[0, 1, 2, X, X, X, X, X], [7, 7, X, X, X, X, X, X], [0, 3, 3, 40, X, X, X, X]]
    # a prefill chunk: the listed sequences relative to its first, their rows of the table, its rows of the segments
    part = ko.rows(1, 3)
    assert _rowlist(part.listed) == ((1,), [1], torch.int32) and part.blocked.tolist() == [[9] * 4]
    assert part.seg.tolist() == ko.seg.tolist()[1:3] and part.layers == (0, 2)
    assert ko.rows(1, 2) is None
    whole = ko.rows(0, 3)
    assert _rowlist(whole.listed)[:2] == ((0, 2), [0, 2]) and whole.blocked.tolist() == ko.blocked.tolist()
    first = ko.rows(0, 2)
    assert _rowlist(first.listed)[:2] == ((0,), [0]) and first.blocked.tolist() == [[4] * 4] and first.seg.shape == (2, 8)


CUT_SEGMENTS = [[0, 0, 1, 1, 2], [0, 1, 3], [31, 2], [0, 0]]
CUT_PLENS = (5, 3, 2, 2)
BITS_1_31 = (1 << 31) | 2


def test_cuts_entries_head_switch_and_the_decode_step_table(cfg):
    """Pairs (1, 0), (2, 1), (2, 31).  Prompt 0: the two positions of segment 1 follow keys of segment 0, the position of segment
    2 keys of segment 1.  Prompt 1: position 1 (segment 1) follows a key of segment 0; segment 3 queries under no pair.  Prompt 2:
    position 1 (segment 2) follows a key of segment 31.  Prompt 3 holds no query segment.  The generated rows query as segment 2,
    2, 2 and as segment 1 in prompt 1: K(2) = {1, 31} meets segment 1 in prompt 0 only and segment 31 in prompt 2 only — a key
    segment the prompt does not hold is no cut — and nothing in prompt 3; K(1) = {0} meets segment 0 in prompt 1."""
    v, probes, ws = _probes(cfg, CUT_PLENS, cuts=dict(segments=CUT_SEGMENTS, pairs=[(1, 0), (2, 1), (2, 31)], layers=(1, 2),
                                                        heads=[3, 1], generated=[2, 1, 2, 2]))
    ct = probes.cuts
    assert [(pos.tolist(), msk.tolist()) for pos, msk in ct.entries] == [([2, 3, 4], [1, 1, BITS_1_31]), ([1], [1]), ([1], [BITS_1_31]), ([], [])]
    assert v.cuts["gen"] == [2, 1, 1 << 31, 0] and v.cuts["generated"] == [2, 1, 2, 2] and v.cuts["heads"] == (1, 3)
    assert v.cuts["pairs"] == [[(1, 0), (2, 1), (2, 31)]] * 4
    assert ct.head_on.tolist() == [0, 1, 0, 1] and ct.head_on.dtype == torch.uint8
    assert ct.seg.tolist() == [[0, 0, 1, 1, 2, X, X, X], [0, 1, 3, X, X, X, X, X], [31, 2, X, X, X, X, X, X], [0, 0, X, X, X, X, X, X]]
    assert (ct.layers, ct.n_layers, ct.tile_rows) == ((1, 2), 2, 4) and ct.covers(1) and not ct.covers(0)
    step = ct.step                                                       # the knockout's operands, heads 1 and 3 alone
    assert step.blocked.tolist() == [[0, 2, 0, 2], [0, 1, 0, 1], [0, BIT31, 0, BIT31]] and step.blocked.dtype == torch.int32
    assert _rowlist(step.listed) == ((0, 1, 2), [0, 1, 2], torch.int32) and step.seg is ct.seg and step.layers == (1, 2)
    assert ct.uid == ("cuts", 3, 1, 2) and probes.graph_key() == (("cuts", 3, 1, 2),) and probes.decode_steps().cuts is ct
    assert sorted(n for n, _ in ws._bufs) == ["gen_ct_blocked", "gen_ct_heads", "gen_ct_rows", "gen_ct_seg"]
    # a prefill chunk: its entries and segment rows, no decode state; None where it lists nothing
    part = ct.rows(1, 3)
    assert [(pos.tolist(), msk.tolist()) for pos, msk in part.entries] == [([1], [1]), ([1], [BITS_1_31])]
    assert part.seg.tolist() == ct.seg.tolist()[1:3] and part.head_on is ct.head_on and part.step is None and part.tile_rows == 4
    assert ct.rows(3, 4) is None and len(ct.rows(0, 4).entries) == 4


def test_cuts_that_leave_the_generated_rows_alone_have_no_decode_state(cfg):
    _, probes, ws = _probes(cfg, CUT_PLENS, cuts=dict(segments=CUT_SEGMENTS, pairs=[(1, 0), (2, 1), (2, 31)], generated=0))
    ct = probes.cuts
    assert ct.step is None and ct.head_on is None and ct.layers == (0, 2) and ct.uid == ("cuts", 0, 0, 2)
    assert probes.decode_steps() is None and probes.graph_key() == ()
    assert sorted(n for n, _ in ws._bufs) == ["gen_ct_seg"]
    # all heads named is all heads: no switch
    _, probes, _ = _probes(cfg, CUT_PLENS, cuts=dict(segments=CUT_SEGMENTS, pairs=[(1, 0)], heads=[0, 1, 2, 3]))
    assert probes.cuts.head_on is None


def _head_vectors(n, n_pairs, D=64):
    """[n, n_pairs, D]: 100 * prompt + index of the pair as given."""
    return (100.0 * torch.arange(n)[:, None, None] + torch.arange(n_pairs)[None, :, None]).expand(n, n_pairs, D).contiguous().float()


def test_head_patch_sorts_its_pairs_and_permutes_its_vectors(cfg):
    """Pairs (1, 2), (0, 1), (1, 0) sort to (0, 1), (1, 0), (1, 2) — the given indices 1, 2, 0 — layer 0 holds pair 0, layer 1
    pairs 1 .. 2; rows [2, 0] ascend to 0, 2."""
    _, probes, ws = _probes(cfg, (3, 2, 4), head_patch=dict(heads=[(1, 2), (0, 1), (1, 0)], vectors=_head_vectors(3, 3), rows=[2, 0],
                                                            mode="add", alpha=0.5, steps="all"))
    hp = probes.head_patch
    assert hp.heads.tolist() == [1, 0, 2] and hp.heads.dtype == torch.int32 and hp.layers == ((0, 0, 1), (1, 1, 3))
    assert hp.pairs(0) == (0, 1) and hp.pairs(1) == (1, 3)
    assert tuple(hp.vectors.shape) == (2, 3, 64) and hp.vectors[:, :, 0].tolist() == [[1.0, 2.0, 0.0], [201.0, 202.0, 200.0]]
    assert bool((hp.vectors == hp.vectors[:, :, :1]).all())
    assert _rowlist(hp.listed) == ((0, 2), [0, 2], torch.int32) and (hp.mode, hp.alpha, hp.steps) == ("add", 0.5, "all")
    assert hp.uid == ("head_patch", 2, 2, ((0, 1), (1, 2)), "add", "all", 0.5) and probes.graph_key() == (hp.uid,)
    assert probes.decode_steps().head_patch is hp
    assert sorted(n for n, _ in ws._bufs) == ["gen_hp_heads", "gen_hp_rows", "gen_hp_vec"]
    part = hp.rows(1, 3)
    assert _rowlist(part.listed) == ((1,), [1], torch.int32) and part.vectors[:, :, 0].tolist() == [[201.0, 202.0, 200.0]]
    assert part.heads is hp.heads and part.layers == hp.layers and part.uid == ("head_patch", 1, 1, ((0, 1), (1, 2)), "add", "all", 0.5)
    assert hp.rows(1, 2) is None


def test_head_patch_shared_vectors(cfg):
    _, probes, _ = _probes(cfg, (3, 2, 4), head_patch=dict(heads=[(1, 2), (0, 1), (1, 0)], vectors=_head_vectors(1, 3)[0]))
    hp = probes.head_patch
    assert tuple(hp.vectors.shape) == (1, 3, 64) and hp.vectors[0, :, 0].tolist() == [1.0, 2.0, 0.0]
    assert _rowlist(hp.listed)[:2] == ((0, 1, 2), [0, 1, 2])
    assert hp.uid == ("head_patch", 3, 1, ((0, 1), (1, 2)), "replace", "prompt", 1.0)
    assert probes.decode_steps() is None and probes.graph_key() == ()          # a patch of the prompt's last row only
    part = hp.rows(1, 3)                                                        # one block for whichever rows are listed
    assert _rowlist(part.listed)[:2] == ((0, 1), [0, 1]) and part.vectors.tolist() == hp.vectors.tolist()


def test_resid_patch_per_prompt_and_shared(cfg):
    vec = torch.arange(3, dtype=torch.float32)[:, None].expand(3, 256).contiguous()
    _, probes, ws = _probes(cfg, (3, 2, 4), patch=dict(site=1, vectors=vec, rows=[2, 1]))
    pt = probes.patch
    assert tuple(pt.vectors.shape) == (2, 256) and pt.vectors[:, 0].tolist() == [1.0, 2.0] and bool((pt.vectors == pt.vectors[:, :1]).all())
    assert _rowlist(pt.listed) == ((1, 2), [1, 2], torch.int32) and (pt.site, pt.mode, pt.alpha, pt.steps) == (1, "replace", 1.0, "prompt")
    assert pt.uid == ("resid_patch", 2, 2, 1, "replace", "prompt", 1.0) and probes.graph_key() == () and probes.decode_steps() is None
    assert sorted(n for n, _ in ws._bufs) == ["gen_rp_rows", "gen_rp_vec"]
    part = pt.rows(0, 2)
    assert _rowlist(part.listed) == ((1,), [1], torch.int32) and part.vectors[:, 0].tolist() == [1.0] and part.site == 1
    assert pt.rows(0, 1) is None and _rowlist(pt.rows(2, 3).listed)[:2] == ((0,), [0]) and pt.rows(2, 3).vectors[:, 0].tolist() == [2.0]
    _, probes, _ = _probes(cfg, (3, 2, 4), patch=dict(site=2, vectors=torch.full((256,), 7.0), mode="add", alpha=0.25, steps="all"))
    pt = probes.patch
    assert tuple(pt.vectors.shape) == (1, 256) and bool((pt.vectors == 7.0).all()) and _rowlist(pt.listed)[:2] == ((0, 1, 2), [0, 1, 2])
    assert pt.uid == ("resid_patch", 3, 1, 2, "add", "all", 0.25) and probes.graph_key() == (pt.uid,) and probes.decode_steps().patch is pt
    assert pt.rows(1, 2).vectors.tolist() == pt.vectors.tolist() and _rowlist(pt.rows(1, 2).listed)[:2] == ((0,), [0])


def test_captures_are_sliced_with_the_chunk(cfg):
    _, probes, ws = _probes(cfg, (3, 2, 4), want_hidden=True, want_heads=True)
    assert tuple(probes.capture.shape) == (3, 3, 256) and probes.capture.dtype == torch.float32
    assert tuple(probes.head_capture.shape) == (3, 2, 4, 64) and probes.head_capture.dtype == torch.bfloat16
    assert sorted(n for n, _ in ws._bufs) == ["gen_head_out", "gen_hidden"]
    part = probes.rows(1, 3)
    assert part.capture.data_ptr() == probes.capture[1:].data_ptr() and tuple(part.capture.shape) == (2, 3, 256)
    assert part.head_capture.data_ptr() == probes.head_capture[1:].data_ptr() and part.knockout is None and part.cuts is None
    assert probes.decode_steps() is None and probes.graph_key() == ()


def test_kept_rows_of_a_drop(cfg):
    """``overlong="drop"`` over prompts 0 and 2 of three (0, 2 and 3 of four for the cuts): each probe keeps the survivors' entries,
    a patch its rows under the indices they have among the survivors."""
    v, _, _ = _probes(cfg, (3, 2, 2), knockout=([[0, 1, 31], [0, 5], [2, 1]], [[31, 1], [0], [1]], None, [0, 2]))
    kept = v.kept([0, 2])
    assert [list(s) for s in kept.knockout["segments"]] == [[0, 1, 31], [2, 1]] and [tuple(b) for b in kept.knockout["blocked"]] == [(1, 31), (1,)]
    assert kept.knockout["layers"] == (0, 2) and kept.knockout["heads"] == (0, 2)
    _, probes, _ = _again(cfg, kept, (3, 2))
    assert probes.knockout.blocked.tolist() == [[-2147483646, 0, -2147483646, 0], [2, 0, 2, 0]] and probes.knockout.listed.seqs == (0, 1)
    assert probes.knockout.seg.tolist() == [[0, 1, 31, X, X, X, X, X], [2, 1, X, X, X, X, X, X]]

    vec = torch.arange(3, dtype=torch.float32)[:, None].expand(3, 256).contiguous()
    v, _, _ = _probes(cfg, (3, 2, 2), want_hidden=True, patch=dict(site=1, vectors=vec, rows=[2, 1], mode="add", alpha=2.0, steps="all"))
    kept = v.kept([0, 2])
    assert kept.patch["rows"] == [1] and kept.patch["vectors"][:, 0].tolist() == [0.0, 2.0] and kept.want_hidden and not kept.want_heads
    assert (kept.patch["site"], kept.patch["mode"], kept.patch["alpha"], kept.patch["steps"]) == (1, "add", 2.0, "all")
    _, probes, _ = _again(cfg, kept, (3, 2))
    assert probes.patch.listed.seqs == (1,) and probes.patch.vectors[:, 0].tolist() == [2.0] and tuple(probes.capture.shape) == (2, 3, 256)
    assert v.kept([0]).patch["rows"] == [] and _again(cfg, v.kept([0]), (3,))[0].patch is None      # no listed row survives: no patch
    shared, _, _ = _probes(cfg, (3, 2, 2), patch=dict(site=0, vectors=torch.full((1, 256), 7.0), rows=[0, 2]))
    assert shared.kept([1, 2]).patch["rows"] == [1] and tuple(shared.kept([1, 2]).patch["vectors"].shape) == (1, 256)

    v, _, _ = _probes(cfg, (3, 2, 2), want_heads=True, head_patch=dict(heads=[(1, 2), (0, 1)], vectors=_head_vectors(3, 2), rows=[1, 2]))
    kept = v.kept([0, 2])
    assert kept.head_patch["rows"] == [1] and kept.head_patch["vectors"][:, :, 0].tolist() == [[0.0, 1.0], [200.0, 201.0]]
    assert kept.head_patch["heads"] == [(1, 2), (0, 1)] and kept.want_heads
    _, probes, _ = _again(cfg, kept, (3, 2))
    assert probes.head_patch.listed.seqs == (1,) and probes.head_patch.vectors[:, :, 0].tolist() == [[201.0, 200.0]]
    assert probes.head_patch.heads.tolist() == [1, 2] and tuple(probes.head_capture.shape) == (2, 2, 4, 64)

    v, _, _ = _probes(cfg, CUT_PLENS, cuts=dict(segments=CUT_SEGMENTS, pairs=[[(1, 0), (2, 1)], [(1, 0)], [(2, 31)], []], layers=(1, 2),
                                                heads=[3, 1], generated=[2, 1, 2, 2]))
    kept = v.kept([0, 2, 3])
    assert sorted(kept.cuts) == ["generated", "heads", "layers", "pairs", "segments"]
    assert [list(s) for s in kept.cuts["segments"]] == [CUT_SEGMENTS[0], CUT_SEGMENTS[2], CUT_SEGMENTS[3]]
    assert kept.cuts["pairs"] == [[(1, 0), (2, 1)], [(2, 31)], []] and kept.cuts["generated"] == [2, 2, 2]
    assert (kept.cuts["layers"], kept.cuts["heads"]) == ((1, 2), (1, 3))
    v2, probes, _ = _again(cfg, kept, (5, 2, 2))
    assert v2.cuts["gen"] == [2, 1 << 31, 0]
    assert [(pos.tolist(), msk.tolist()) for pos, msk in probes.cuts.entries] == [([2, 3, 4], [1, 1, 2]), ([1], [1 << 31]), ([], [])]
    assert probes.cuts.step.blocked.tolist() == [[0, 2, 0, 2], [0, BIT31, 0, BIT31]] and probes.cuts.step.listed.seqs == (0, 1)
    assert probes.cuts.uid == ("cuts", 2, 1, 2)

"""Attention cuts between prompt segments above the kernel, without a GPU: what ``generate(cuts=)`` refuses before anything is
sized or launched; the listing rule and the tile tables; what it launches, traced on ``meta`` tensors through
tests/tools/launch_trace.py (imported, not edited) on a head_dim-64 decoder (tiles of four rows), a grouped-query one (tiles of one)
and one with the trimmed last layer; what keys its captured decode graphs; and the entry point's own refusals through ctypes."""
import ast
import contextlib
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import launch_trace as lt  # noqa: E402

CONFIGS = ("tiny_h4", "7b_gqa8_bias", "7b_lora")      # head_dim 64, R = 4, untrimmed; G = 4, R = 1, untrimmed; R = 4, trimmed last layer
TILE_ROWS = {"tiny_h4": 4, "7b_gqa8_bias": 1, "7b_lora": 4}
PAIRS = [(1, 0), (2, 1)]


def _cuts(lens=lt.GEN_LENS, pairs=PAIRS, **kw):
    return dict(segments=lt.segments_of(lens), pairs=pairs, **kw)


def _pairs_of(entries):
    """A validated prompt's (positions, masks) arrays as a list of (p, mask)."""
    return [list(zip(pos.tolist(), msk.tolist())) for pos, msk in entries]


def _listed(seg, K):
    """Brute force: position p is listed iff a key j <= p has seg[j] in K(seg[p]); with its bit set."""
    return [(p, sum(1 << g for g in K.get(s, ()))) for p, s in enumerate(seg) if any(seg[j] in K.get(s, ()) for j in range(p + 1))]


# ---- host validation ----------------------------------------------------------------------------------------------------
def _bare_runtimes():
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.qwen import QwenAudioRuntime
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    cfg = SalmonnCfg.tiny().llama
    for cls in (SalmonnRuntime, QwenAudioRuntime):
        rt = object.__new__(cls)            # no weights, no workspace, no device: anything past the validation raises AttributeError
        rt.lm_cfg, rt.llama, rt.ws, rt.device, rt.kv_dtype = cfg, None, None, torch.device("cpu"), "bf16"
        yield rt


def _refusals(n_layers, n_heads):
    ok = _cuts((3, 2, 4))
    return ok, {
        "unknown keys": dict(ok, blocked=[[1]]),
        "must be a dict": (ok["segments"], PAIRS),
        "'segments' and 'pairs'": [dict(pairs=PAIRS), dict(segments=ok["segments"])],
        "segment lists for 3 prompts": dict(ok, segments=ok["segments"][:2]),
        "positions": dict(ok, segments=[[0, 1], [0, 1], [0, 1, 2, 3]]),
        "0..255": [dict(ok, segments=[[0, 1, 256], [0, 1], [0, 1, 2, 3]]), dict(ok, segments=[[0, -1, 2], [0, 1], [0, 1, 2, 3]])],
        "0..31": [dict(ok, pairs=[(32, 0)]), dict(ok, pairs=[(1, 32)]), dict(ok, pairs=[(-1, 0)]), dict(ok, pairs=[[(1, 0)], [], [(0, 40)]])],
        "pairs": [dict(ok, pairs=5), dict(ok, pairs=[(1, 0, 2)]), dict(ok, pairs=[[(1, 0)], []]), dict(ok, pairs=[[1, 0], [(1, 0)], 3])],
        "layer window": [dict(ok, layers=(0, n_layers + 1)), dict(ok, layers=(1, 1)), dict(ok, layers=(-1, 1))],
        "layers must be": [dict(ok, layers=1), dict(ok, layers=(0, 1, 2))],
        "head indices": [dict(ok, heads=[n_heads]), dict(ok, heads=[-1]), dict(ok, heads=[])],
        "heads must be": dict(ok, heads=3),
        "generated": [dict(ok, generated=256), dict(ok, generated=[1, 2]), dict(ok, generated="x"), dict(ok, generated=[1, 2, -1])],
        "prompt 2, position 0": dict(ok, segments=[[0, 1, 2], [0, 2], [1, 1, 0, 2]], pairs=[(1, 1)]),     # its first key is its own
    }


@pytest.mark.parametrize("rt", list(_bare_runtimes()), ids=["salmonn", "qwen-audio"])
def test_generate_refuses_bad_cuts_in_both_runtimes(rt):
    c = rt.lm_cfg
    rt.kv_dtype = "bf16"
    prompts = [[[3, 4, 5]], [[6, 7]], [[8, 9, 10, 11]]]
    ok, refusals = _refusals(c.n_layers, c.n_heads)
    gen = lambda ct, **kw: rt.generate(prompts, None, max_new_tokens=2, cuts=ct, **kw)
    for word, cts in refusals.items():
        for ct in (cts if isinstance(cts, list) else [cts]):
            with pytest.raises(ValueError, match="cuts.*" + word):
                gen(ct)
    with pytest.raises(ValueError, match="prompt 0, position 0"):
        gen(dict(ok, pairs=[(0, 0)]))
    with pytest.raises(ValueError, match="cuts.*num_beams"):
        gen(ok, num_beams=2)
    rt.kv_dtype = "fp8"
    with pytest.raises(ValueError, match="cuts needs the bf16 KV cache"):
        gen(ok)
    rt.kv_dtype = "bf16"
    with pytest.raises(ValueError, match="cuts together with knockout"):
        gen(ok, knockout=([[0] * 3, [0, 1], [0] * 4], [[], [1], []]))
    with pytest.raises(ValueError, match="cuts together with knockout, patch or head_patch"):
        gen(ok, patch=dict(site=1, vectors=torch.zeros(3, c.hidden)))
    with pytest.raises(ValueError, match="cuts together with knockout, patch or head_patch"):
        gen(ok, head_patch=dict(heads=[(0, 0)], vectors=torch.zeros(1, c.head_dim)))
    for good in (ok, dict(ok, generated=2), dict(ok, generated=[1, 255, 40], heads=[0], layers=(0, 1)), dict(ok, pairs=[PAIRS, [], PAIRS]),
                 dict(ok, pairs=[]), dict(ok, pairs=[(5, 6)])):             # the last two list nothing: the plain call
        with pytest.raises(AttributeError):                                 # past the validation: the first launch
            gen(good)
    with pytest.raises(AttributeError):                                     # cuts that list nothing go with a knockout
        gen(dict(ok, pairs=[(5, 6)]), knockout=([[0] * 3, [0, 1], [0] * 4], [[], [1], []]))


def test_the_listing_rule():
    from icl_speech_text_llm_amd.runtime import probes as P
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    cfg = SalmonnCfg.tiny().llama
    g = torch.Generator().manual_seed(3)
    segs = [torch.randint(0, 6, (n,), generator=g).tolist() for n in (1, 7, 40)] + [[0, 0, 40, 1, 255, 1, 33, 2]]
    pairs = [(1, 0), (2, 1), (3, 3), (5, 2), (5, 0)]
    K = {}
    for a, b in pairs:
        K.setdefault(a, set()).add(b)
    # (3, 3): a query that does not read its own segment is listed from the segment's first position on; every prompt starts with
    # a key of segment 0, which segment 3 may read, so no row is left without a key
    segs = [[0] + s for s in segs]
    check = lambda cuts, plens=[len(s) for s in segs]: P.check_probes(cfg, "bf16", plens, 1, cuts=cuts).cuts
    all_of = P.check_probes(cfg, "bf16", [len(s) for s in segs], 1, cuts=dict(segments=segs, pairs=pairs))
    v = all_of.cuts
    assert _pairs_of(v["entries"]) == [_listed(s, K) for s in segs]
    assert any(_pairs_of(v["entries"])) and v["layers"] == (0, cfg.n_layers) and v["heads"] is None
    # per-prompt pairs; ids >= 32 and 255 are never cut (40 is not 8 mod 32) and never a query segment
    per = check(dict(segments=segs, pairs=[pairs, [], [(1, 0)], [(1, 8), (8, 1), (2, 0)]]))
    assert _pairs_of(per["entries"]) == [_listed(segs[0], K), [], _listed(segs[2], {1: {0}}), _listed(segs[3], {2: {0}})]
    # generated: None = the segment of the last position; an id >= 32 or without pairs = 0; a key segment the prompt lacks = no cut
    assert v["gen"] == [sum(1 << g for g in K.get(s[-1], ()) if g in s) for s in segs]
    assert check(dict(segments=segs, pairs=pairs, generated=255))["gen"] == [0] * 4
    assert check(dict(segments=segs, pairs=[(9, 0)], generated=9))["gen"] == [1] * 4
    assert check(dict(segments=segs, pairs=[(9, 0)], generated=[9, 0, 255, 9]))["gen"] == [1, 0, 0, 1]
    assert check(dict(segments=segs, pairs=[(9, 20)], generated=9)) is None
    # a validated dict is itself a valid argument, with the same result (overlong="drop" hands it on)
    again = check({k: v[k] for k in P.CUT_KEYS})
    assert _pairs_of(again["entries"]) == _pairs_of(v["entries"]) and {k: again[k] for k in again if k not in ("entries", "segments")} == {k: v[k] for k in v if k not in ("entries", "segments")}
    assert [sg.tolist() for sg in again["segments"]] == segs
    kept = check(all_of.kept([1, 3]).cuts, [len(segs[1]), len(segs[3])])
    assert _pairs_of(kept["entries"]) == [_pairs_of(v["entries"])[1], _pairs_of(v["entries"])[3]] and kept["gen"] == [v["gen"][1], v["gen"][3]]


@pytest.mark.parametrize("R", [1, 2, 4])
def test_tile_tables(R):
    import numpy as np
    from icl_speech_text_llm_amd.runtime.probes import Cuts
    entries = (((2, 1), (3, 1), (4, 6), (6, 1 << 31), (7, 2)), (), ((0, 1),), ((1, 4), (2, 4), (3, 4), (4, 4)))
    arrays = lambda ents: tuple((np.array([p for p, _ in e], dtype=np.int64), np.array([m for _, m in e], dtype=np.int64)) for e in ents)
    seq_lens, cu = [8, 3, 1, 5], [0, 8, 11, 12]
    ct = Cuts(torch.zeros(4, 8, dtype=torch.uint8), arrays(entries), (0, 3), 3, R)
    (tables,) = ct.tile_tables(seq_lens, cu, False, "cpu")
    tile_seq, row_q, row_len, blocked = (t.tolist() for t in tables)
    assert len(row_q) == len(row_len) == len(blocked) == R * len(tile_seq)
    assert tile_seq == sorted(tile_seq) and [tile_seq.count(b) for b in range(4)] == [-(-len(e) // R) for e in entries]
    live = [(tile_seq[i // R], q, n, m) for i, (q, n, m) in enumerate(zip(row_q, row_len, blocked)) if q >= 0]
    assert live == [(b, cu[b] + p, p + 1, m - (1 << 32) if m >= 1 << 31 else m) for b, e in enumerate(entries) for p, m in e]   # ascending
    for t in range(len(tile_seq)):                           # empty slots only at the tail of a tile, zeroed
        qs = row_q[t * R:(t + 1) * R]
        k = sum(q >= 0 for q in qs)
        assert k >= 1 and all(q >= 0 for q in qs[:k]) and qs[k:] == [-1] * (R - k)
        assert row_len[t * R + k:(t + 1) * R] == [0] * (R - k) and blocked[t * R + k:(t + 1) * R] == [0] * (R - k)
    # the last layer: only listed last rows (sequences 0, 2 and 3), packed or gathered rows
    (last,) = ct.tile_tables(seq_lens, cu, True, "cpu")
    assert last[0].tolist() == [0, 2, 3] and [q for q in last[1].tolist() if q >= 0] == [7, 11, 16] and [n for n in last[2].tolist() if n] == [8, 1, 5]
    (gathered,) = ct.tile_tables(seq_lens, None, True, "cpu")
    assert [q for q in gathered[1].tolist() if q >= 0] == [0, 2, 3] and len(gathered[1]) == 3 * R
    assert Cuts(None, arrays(((), ((0, 1),), (), ())), (0, 3), 3, R).tile_tables(seq_lens, None, True, "cpu") == []
    # more tiles than a launch holds: several launches, in order
    parts = ct.tile_tables(seq_lens, cu, False, "cpu", max_tiles=2)
    assert [len(p[0]) for p in parts] == [2] * (len(tile_seq) // 2) + [1] * (len(tile_seq) % 2)
    assert [x for p in parts for x in p[1].tolist()] == row_q and [x for p in parts for x in p[0].tolist()] == tile_seq
    # rows(): a chunk's entries under sequence ids relative to it; None where it lists nothing
    assert ct.rows(1, 2) is None and _pairs_of(ct.rows(1, 3).entries) == [list(e) for e in entries[1:3]] and len(ct.rows(0, 4).entries) == 4


# ---- the launches ---------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _traced(cname, kv="bf16", **attrs):
    if not lt.device_ok():
        pytest.skip(f"the trace is taken at {lt.N_CU} CUs (MI355X); this device has another count")
    rec = lt.Recorder()
    with lt.generate_recording(rec):
        rt = lt.generate_runtime(cname, kv, rec)
        rt.phase_marks = None
        for k, v in attrs.items():
            setattr(rt, k, v)
        yield rt, rec


def _log(cname, lens=lt.GEN_LENS, attrs=None, **kw):
    with _traced(cname, **(attrs or {})) as (rt, rec):
        lens = lens(rt.lm_cfg) if callable(lens) else lens
        kw = {k: v(lens) if callable(v) else v for k, v in kw.items()}
        res = rt.generate(lt.prompts_of(lens), None, **{"max_new_tokens": 4, **kw})
        return list(rec.log), res, rt.lm_cfg


def _names(log, drop=()):
    return [n for n in (l.split("(")[0] for l in log) if n not in drop]


def _cut_launches(log):
    """[(row_q, row_len, tile_seq, blocked, the line)] of every attn_cut_rows launch."""
    out = []
    for l in log:
        if l.startswith("attn_cut_rows("):
            val = lambda name: ast.literal_eval(re.search(name + r"=i32(\[[^\]]*\])", l).group(1))
            out.append((val("row_q"), val("row_len"), val("tile_seq"), val("blocked"), l))
    return out


@pytest.mark.parametrize("cname", CONFIGS[:2])
def test_every_refusal_comes_with_an_empty_launch_log(cname):
    with _traced(cname) as (rt, rec):
        c = rt.lm_cfg
        ok = _cuts()
        cases = [dict(cuts=dict(ok, pairs=[(32, 0)])), dict(cuts=dict(ok, layers=(0, 9))), dict(cuts=dict(ok, generated=256)),
                 dict(cuts=dict(ok, pairs=[(0, 0)])), dict(cuts=ok, num_beams=2), dict(cuts=ok, patch=dict(site=1, vectors=torch.zeros(5, c.hidden))),
                 dict(cuts=ok, knockout=(lt.segments_of(lt.GEN_LENS), [[1], [], [], [], []])), dict(cuts=dict(ok, heads=[c.n_heads]))]
        for kw in cases:
            with pytest.raises(ValueError):
                rt.generate(lt.prompts_of(), None, max_new_tokens=3, **kw)
            assert rec.log == [] and rec.requests == {}, kw


@pytest.mark.parametrize("cname", CONFIGS)
def test_without_cuts_and_with_cuts_that_list_nothing_the_plain_call_is_launched(cname):
    plain, _, _ = _log(cname)
    assert _log(cname, cuts=None)[0] == plain
    assert _log(cname, cuts=_cuts(pairs=[]))[0] == plain
    assert _log(cname, cuts=_cuts(pairs=[(0, 1), (5, 0), (3, 7)]))[0] == plain       # no query of segment 0 has a key of 1 before it
    assert _log(cname, cuts=_cuts(pairs=[(0, 3)], generated=3))[0] == plain            # ... nor of 3, and K(3) is empty
    assert not _cut_launches(plain)


@pytest.mark.parametrize("chunk,chunks", [(128, [(0, 5)]), (2, [(0, 2), (2, 4), (4, 5)])])
@pytest.mark.parametrize("cname", CONFIGS)
def test_interior_cuts_launch_once_per_windowed_layer_and_chunk_but_not_in_the_last_layer(cname, chunk, chunks):
    """Pairs (1, 0), (2, 1) on four segment runs: the last position of every prompt (segment 3) is not listed, so the model's last
    layer launches nothing, and the generated rows (``generated`` None: segment 3) are the plain ones."""
    attrs = dict(prefill_chunk=chunk)
    plain, _, c = _log(cname, attrs=attrs)
    log, _, _ = _log(cname, attrs=attrs, cuts=_cuts())
    R, lens, segs = TILE_ROWS[cname], lt.GEN_LENS, lt.segments_of(lt.GEN_LENS)
    launches = _cut_launches(log)
    assert len(launches) == (c.n_layers - 1) * len(chunks)
    K = {1: {0}, 2: {1}}
    for (row_q, row_len, tile_seq, blocked, line), (b0, b1) in zip(launches, chunks * (c.n_layers - 1)):
        cu, want = 0, []
        for b in range(b0, b1):
            want += [(b - b0, cu + p, p + 1, m) for p, m in _listed(segs[b], K)]
            cu += lens[b]
        live = [(tile_seq[i // R], q, n, m) for i, (q, n, m) in enumerate(zip(row_q, row_len, blocked)) if q >= 0]
        assert live == want and len(row_q) == R * len(tile_seq)
        assert f"tile_rows={R}" in line and "head_on=None" in line and f"n_kv_heads={c.kv_heads}" in line
    # ... and nothing else changes: the same launches otherwise (one copy fills the segment table), the decode steps the plain ones
    names = _names(log, drop=("attn_cut_rows",))
    assert names[1] == "torch.copy_" and names[:1] + names[2:] == _names(plain)
    for i, n in enumerate(_names(log)):
        if n == "attn_cut_rows":
            assert _names(log)[i - 1] == "attn_fwd" and _names(log)[i + 1] in ("gemm", "gemm_rmsnorm")
    assert "attn_decode_masked" not in _names(log)


@pytest.mark.parametrize("cname", CONFIGS)
def test_the_last_layer_launches_listed_last_rows_only(cname):
    """Pairs (3, 0), (1, 0) in all layers: interior rows of segment 1 and the last rows (segment 3).  The first layer launches
    all of them, the model's last layer one tile per sequence with its last row alone — the gathered row where that layer is
    trimmed — and the decode steps the knockout's launch for every sequence (``generated`` None: segment 3)."""
    log, _, c = _log(cname, cuts=_cuts(pairs=[(3, 0), (1, 0)], heads=[0, 2]))
    R, lens, segs = TILE_ROWS[cname], lt.GEN_LENS, lt.segments_of(lt.GEN_LENS)
    first, last = _cut_launches(log)
    cu = [sum(lens[:b]) for b in range(5)]
    assert [q for q in first[0] if q >= 0] == [cu[b] + p for b in range(5) for p, _ in _listed(segs[b], {3: {0}, 1: {0}})]
    trimmed = cname == "7b_lora"
    assert [q for q in last[0] if q >= 0] == ([0, 1, 2, 3, 4] if trimmed else [cu[b] + lens[b] - 1 for b in range(5)])
    assert [n for n in last[1] if n] == list(lens) and last[2] == [0, 1, 2, 3, 4] and len(last[0]) == 5 * R
    assert "head_on=T" in first[4] and "head_on=T" in last[4]
    steps = [l for l in log if l.startswith("attn_decode_masked(")]
    assert len(steps) == c.n_layers * 3 and all("row_seq=T" in l for l in steps)
    assert "attn_decode_rope" not in _names(log)
    # window (1, 2) = the last layer alone: the first launch goes, with an interior-only list nothing is launched at all in the prefill
    only_last, _, _ = _log(cname, cuts=_cuts(pairs=[(3, 0), (1, 0)], layers=(1, 2)))
    assert [x[:4] for x in _cut_launches(only_last)] == [last[:4]]
    interior, _, _ = _log(cname, cuts=_cuts(layers=(1, 2)))
    assert not _cut_launches(interior) and "attn_decode_masked" not in _names(interior)


@pytest.mark.parametrize("cname", CONFIGS[:2])
def test_overlong_drop_hands_the_survivors_lists_on(cname):
    pairs = [[(1, 0)], [(2, 1)], [(1, 0), (2, 0), (3, 0)], [(3, 1)], []]
    log, res, c = _log(cname, lens=lt._overlong_third, overlong="drop", cuts=lambda lens: dict(segments=lt.segments_of(lens), pairs=pairs, generated=[3, 3, 3, 3, 3]))
    alone, _, _ = _log(cname, lens=(5, 9, 4, 6), cuts=lambda lens: dict(segments=lt.segments_of(lens), pairs=pairs[:2] + pairs[3:], generated=3))
    assert res.dropped == (2,)
    assert [x[:4] for x in _cut_launches(log)] == [x[:4] for x in _cut_launches(alone)] and len(_cut_launches(log)) == 2
    steps = [l for l in log if l.startswith("attn_decode_masked(")]
    assert len(steps) == c.n_layers * 3                      # prompt 3 of the call, (3, 1), is the survivors' prompt 2
    vals = [m.group(1) for l in log if l.startswith("torch.copy_(") for m in [re.search(r"host:int32(\[[^a-zA-Z]*\])", l)] if m]
    assert "[2]" in vals


class FakeGraphs:
    """torch.cuda.CUDAGraph / torch.cuda.graph / torch.cuda.synchronize: ``graph`` runs its body once; a graph counts its replays."""

    def __init__(self, monkeypatch):
        self.replays = 0
        outer = self

        class Graph:
            def replay(self):
                outer.replays += 1

        @contextlib.contextmanager
        def graph(g):
            assert isinstance(g, Graph)
            yield
        monkeypatch.setattr(torch.cuda, "CUDAGraph", Graph)
        monkeypatch.setattr(torch.cuda, "graph", graph)
        monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)


def test_graph_keys_of_cuts(monkeypatch):
    """What keys a decode graph under cuts: their uid — the number of sequences listed in the decode steps and the layer window —
    appended to the key of the plain call; nothing of the prefill's lists.  Cuts that leave the generated rows alone replay the
    plain graph."""
    fake = FakeGraphs(monkeypatch)
    with _traced("tiny_h4", use_graphs=True) as (rt, rec):
        rt._graph_reset()
        c = rt.lm_cfg

        def run(**kw):
            """(replays, graphs kept) after one call"""
            r = fake.replays
            rt.generate(lt.prompts_of(), None, max_new_tokens=3, **kw)
            return fake.replays - r, len(rt._graphs)

        assert [run() for _ in range(2)] == [(0, 0), (1, 1)]
        (plain,) = rt._graphs
        assert plain == (5, 64, 2, c.eos_id, c.pad_id, None, False, "bf16")
        # interior cuts, generated rows untouched (None: segment 3; 255; a segment without pairs): the plain graph replays
        assert run(cuts=_cuts()) == (1, 1) and run(cuts=_cuts(generated=255)) == (1, 1) and run(cuts=_cuts(generated=0)) == (1, 1)
        assert [run(cuts=_cuts(generated=1)) for _ in range(2)] == [(0, 1), (1, 2)]
        assert list(rt._graphs)[1] == plain + (("cuts", 5, 0, 2),)
        # other pairs, other heads, other prefill lists with the same number of sequences in the decode steps replay
        assert run(cuts=_cuts(pairs=[(2, 0), (2, 1), (3, 2)], generated=2, heads=[1])) == (1, 2)
        assert run(cuts=_cuts(pairs=[(3, 0)])) == (1, 2)                                  # generated None = segment 3
        # another count of listed sequences and another window capture anew
        assert [run(cuts=_cuts(generated=[1, 255, 1, 1, 0])) for _ in range(2)] == [(0, 2), (1, 3)]
        assert list(rt._graphs)[2] == plain + (("cuts", 3, 0, 2),)
        assert [run(cuts=_cuts(generated=1, layers=(1, 2))) for _ in range(2)] == [(0, 3), (1, 4)]
        assert list(rt._graphs)[3] == plain + (("cuts", 5, 1, 2),)


# ---- the entry point ------------------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_bad_arguments():
    """Every condition attn_decode_check (csrc/attn_decode.hip) tests for the row-tile form, through ctypes: ICL_EINVAL and a
    message that starts with the entry point and names the condition.  The pointers are made up, so every call has to return
    before a launch — which is why this never runs where a GPU could take one."""
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: a check that wrongly passed would launch on them")
    import icl_speech_text_llm_amd.runtime.binding as b
    lib = b.load_library()
    assert {"icl_attn_cut_tile_rows", "icl_attn_cut_rows_bf16"} <= set(b.EXPORTED_SYMBOLS) and b.ABI_VERSION == 6
    assert [lib.icl_attn_cut_tile_rows(*a) for a in ((32, 32, 128), (32, 0, 128), (4, 4, 64), (32, 16, 128), (32, 8, 128), (32, 4, 128))] == [4, 4, 4, 2, 1, 1]
    assert [lib.icl_attn_cut_tile_rows(*a) for a in ((32, 2, 128), (8, 4, 64), (32, 5, 128), (4, 4, 96), (0, 0, 128), (4, -1, 128))] == [-1] * 6
    assert [b.attn_cut_tile_rows(32, 128), b.attn_cut_tile_rows(32, 128, 16)] == [4, 2]
    with pytest.raises(b.IclError, match="icl_attn_cut_tile_rows"):
        b.attn_cut_tile_rows(8, 64, 4)
    H, D = 32, 128
    names = "Q ldq Kc Vc O ldo seg ld_seg tile_seq row_q row_len blocked head_on n_tiles tile_rows n_heads n_kv_heads head_dim max_len scale stream".split()
    sizes = dict(ldq=H * D, ldo=H * D, ld_seg=64, n_tiles=3, tile_rows=1, n_heads=H, n_kv_heads=8, head_dim=D, max_len=64, scale=D ** -0.5, stream=None)
    base = {n: sizes[n] if n in sizes else (i + 1) << 20 for i, n in enumerate(names)}
    cases = [(n + " NULL", "NULL pointer", {n: None}) for n in names if n not in sizes and n != "head_on"]
    cases += [
        ("no tiles", "bad sizes: n_tiles=0", dict(n_tiles=0)), ("65536 tiles", "bad sizes: n_tiles=65536", dict(n_tiles=65536)),
        ("n_heads 0", "bad sizes", dict(n_heads=0)), ("max_len 0", "bad sizes", dict(max_len=0)),
        ("tile_rows 4 at G = 4", "tile_rows=4, the form's tiles hold 1 rows", dict(tile_rows=4)),
        ("tile_rows 1 at G = 1", "tile_rows=1, the form's tiles hold 4 rows", dict(n_kv_heads=0)),
        ("tile_rows 1 at G = 2", "tile_rows=1, the form's tiles hold 2 rows", dict(n_kv_heads=16)),
        ("tile_rows 0", "tile_rows=0", dict(tile_rows=0)),
        ("head_dim 96", "head_dim=96 (only 64 and 128)", dict(head_dim=96)),
        ("32 % 5", "is not a multiple of n_kv_heads=", dict(n_kv_heads=5)), ("n_kv_heads -1", "is not a multiple of n_kv_heads=", dict(n_kv_heads=-1)),
        ("G = 16", "16 query heads per K/V head (G at most 8)", dict(n_kv_heads=2)),
        ("G = 4 at head_dim 64", "head_dim=64 (grouped-query attention: only 128)", dict(head_dim=64)),
        ("ld_seg < max_len", "ld_seg=63 < max_len=64", dict(ld_seg=63)),
        ("ldq < n_heads * head_dim", "ldq=4088 / ldo=4096 must hold n_heads * head_dim = 4096 columns", dict(ldq=H * D - 8)),
        ("ldo < n_heads * head_dim", "ldq=4096 / ldo=4088 must hold", dict(ldo=H * D - 8)),
        ("ldq % 8", "misaligned operands", dict(ldq=H * D + 4)), ("blocked + 2 bytes", "misaligned operands", dict(blocked=base["blocked"] + 2)),
        ("scale inf", "scale is not finite", dict(scale=float("inf"))), ("scale nan", "scale is not finite", dict(scale=float("nan"))),
    ] + [(n + " + 8 bytes", "misaligned operands", {n: base[n] + 8}) for n in ("Q", "Kc", "Vc")]
    for what, words, broken in cases:
        assert set(broken) <= set(base), what
        rc = lib.icl_attn_cut_rows_bf16(*[{**base, **broken}[n] for n in names])
        msg = (lib.icl_last_error() or b"").decode()
        assert rc == -1 and msg.startswith("icl_attn_cut_rows_bf16: ") and words in msg, (what, rc, msg)

"""Attention-head output capture and patching above the kernel, without a GPU: what ``generate(want_heads=, head_patch=)`` refuses
before anything is sized or launched; what it launches, traced on ``meta`` tensors through tests/tools/launch_trace.py (imported,
not edited) on a head_dim-64, a grouped-query and a trimmed-last-layer decoder; and what keys its captured decode graphs, with a
stand-in for the graph API as tests/test_launch_trace.py::test_graph_keys_of_the_probes does."""
import ast
import contextlib
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import launch_trace as lt  # noqa: E402

CONFIGS = ("tiny_h4", "7b_gqa8_bias", "7b_lora")      # head_dim 64 untrimmed; grouped-query untrimmed; the trimmed last layer


# ---- host validation ----------------------------------------------------------------------------------------------------
def _bare_runtimes():
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.qwen import QwenAudioRuntime
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    cfg = SalmonnCfg.tiny().llama
    for cls in (SalmonnRuntime, QwenAudioRuntime):
        rt = object.__new__(cls)            # no weights, no workspace, no device: anything past the validation raises AttributeError
        rt.lm_cfg, rt.llama, rt.ws, rt.device = cfg, None, None, torch.device("cpu")
        yield rt


def _refusals(c, n=3):
    D = c.head_dim
    vec = torch.zeros(n, 2, D)
    ok = dict(heads=[(1, 0), (0, c.n_heads - 1)], vectors=vec)
    return ok, {
        "unknown": dict(ok, site=1),
        "dict": (ok["heads"], vec),
        "'heads' and 'vectors'": [dict(vectors=vec), dict(heads=ok["heads"])],
        "outside": [dict(ok, heads=[(1, 0), (c.n_layers, 0)]), dict(ok, heads=[(1, 0), (0, c.n_heads)]), dict(ok, heads=[(-1, 0), (0, 0)]),
                    dict(ok, heads=[(0, -1), (0, 0)]), dict(ok, rows=[0, n]), dict(ok, rows=[-1])],
        "pair twice": dict(ok, heads=[(1, 0), (1, 0)]),
        "pairs": [dict(ok, heads=[1, 0]), dict(ok, heads=5)],
        "empty": dict(ok, heads=[], vectors=torch.zeros(n, 0, D)),
        "float32": [dict(ok, vectors=vec.double()), dict(ok, vectors=vec.to(torch.bfloat16)), dict(ok, vectors=[[0.0] * D] * 2)],
        "shape": [dict(ok, vectors=torch.zeros(n - 1, 2, D)), dict(ok, vectors=torch.zeros(n, 3, D)), dict(ok, vectors=torch.zeros(n, 2, D + 8)),
                  dict(ok, vectors=torch.zeros(D)), dict(ok, vectors=torch.zeros(1, n, 2, D)), dict(ok, vectors=torch.zeros(3, D))],
        "mode": [dict(ok, mode="mul"), dict(ok, mode=0)],
        "steps": [dict(ok, steps="decode"), dict(ok, steps=None)],
        "alpha": [dict(ok, mode="add", alpha=float("nan")), dict(ok, mode="add", alpha=float("inf")), dict(ok, alpha="x")],
        "prompt twice": dict(ok, rows=[0, 2, 0]),
        "rows must be": dict(ok, rows=1),
    }


@pytest.mark.parametrize("rt", list(_bare_runtimes()), ids=["salmonn", "qwen-audio"])
def test_generate_refuses_a_bad_head_patch_in_both_runtimes(rt):
    c = rt.lm_cfg
    prompts = [[[3, 4, 5]], [[6, 7]], [[8, 9, 10, 11]]]
    ok, refusals = _refusals(c)
    gen = lambda hp, **kw: rt.generate(prompts, None, max_new_tokens=2, head_patch=hp, **kw)
    for word, hps in refusals.items():
        for hp in (hps if isinstance(hps, list) else [hps]):
            with pytest.raises(ValueError, match="head_patch.*" + word):
                gen(hp)
    with pytest.raises(ValueError, match="head_patch.*num_beams"):
        gen(ok, num_beams=2)
    with pytest.raises(ValueError, match="want_heads.*num_beams"):
        rt.generate(prompts, None, max_new_tokens=2, want_heads=True, num_beams=2)
    with pytest.raises(ValueError, match="head_patch together with knockout"):
        gen(ok, knockout=([[0] * 3, [0, 1], [0] * 4], [[], [1], []]))
    with pytest.raises(ValueError, match="head_patch together with knockout or with patch"):
        gen(ok, patch=dict(site=1, vectors=torch.zeros(3, c.hidden)))
    for good in (dict(ok, rows=[2, 0], mode="add", alpha=0.5, steps="all"), dict(ok, rows=[]),      # an empty list: no patch
                 dict(ok, vectors=torch.zeros(2, c.head_dim)), dict(ok, vectors=torch.zeros(1, 2, c.head_dim))):
        with pytest.raises(AttributeError):         # past the validation: the first launch
            gen(good)
    with pytest.raises(AttributeError):             # an all-empty knockout is no knockout
        gen(ok, knockout=([[0] * 3, [0, 1], [0] * 4], [[], [], []]))
    with pytest.raises(ValueError, match="head_out must be"):
        rt.head_contrib(torch.zeros(3, c.n_layers, c.n_heads, c.head_dim), [(0, 0)])
    with pytest.raises(ValueError, match="head_contrib.*outside"):
        rt.head_contrib(torch.zeros(3, c.n_layers, c.n_heads, c.head_dim, dtype=torch.bfloat16), [(c.n_layers, 0)])


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


@pytest.mark.parametrize("cname", CONFIGS[:2])
def test_every_refusal_comes_with_an_empty_launch_log(cname):
    with _traced(cname) as (rt, rec):
        c = rt.lm_cfg
        ok, refusals = _refusals(c, n=5)
        cases = [hp for hps in refusals.values() for hp in (hps if isinstance(hps, list) else [hps])]
        for kw in ([dict(head_patch=hp) for hp in cases] + [dict(head_patch=ok, num_beams=2), dict(want_heads=True, num_beams=2),
                   dict(head_patch=ok, patch=dict(site=1, vectors=torch.zeros(5, c.hidden))),
                   dict(head_patch=ok, knockout=(lt.segments_of(lt.GEN_LENS), [[1], [], [], [], []]))]):
            with pytest.raises(ValueError):
                rt.generate(lt.prompts_of(), None, max_new_tokens=3, **kw)
            assert rec.log == [] and rec.requests == {}, kw


# ---- the launches ---------------------------------------------------------------------------------------------------------
def _log(cname, lens=lt.GEN_LENS, kv="bf16", attrs=None, **kw):
    with _traced(cname, kv, **(attrs or {})) as (rt, rec):
        lens = lens(rt.lm_cfg) if callable(lens) else lens
        kw = {k: v(rt.lm_cfg) if callable(v) else v for k, v in kw.items()}
        res = rt.generate(lt.prompts_of(lens), None, **{"max_new_tokens": 4, **kw})
        return list(rec.log), res, rt.lm_cfg


def _names(log, drop=()):
    return [n for n in (l.split("(")[0] for l in log) if n not in drop]


def _but_for_the_patch(log):
    """The names without the head_rows launches and without the three copies that fill the patch's buffers, which come first
    after the prompt's embedding (the vectors, the head list, the row list)."""
    names = _names(log, drop=("head_rows",))
    assert names[1:4] == ["torch.copy_"] * 3, names[:5]
    return names[:1] + names[4:]


def _head_rows(log):
    return [l for l in log if l.startswith("head_rows(")]


def _hp(pairs, rows=None, steps="prompt", fill=None, n=5, **kw):
    def make(c):
        vec = torch.zeros(n, len(pairs), c.head_dim)
        if fill is not None:
            vec += torch.tensor(fill, dtype=torch.float32)[:, None, None]
        return dict(heads=pairs, vectors=vec, rows=rows, steps=steps, **kw)
    return make


@pytest.mark.parametrize("cname", CONFIGS)
def test_without_the_arguments_nothing_new_is_launched(cname):
    plain, res, _ = _log(cname)
    same, res2, _ = _log(cname, want_heads=False, head_patch=None)
    empty, _, _ = _log(cname, head_patch=_hp([(0, 1)], rows=[]))
    assert plain == same == empty and not _head_rows(plain)
    assert res.head_out is None and res2.head_out is None


@pytest.mark.parametrize("chunk,n_chunks", [(128, 1), (2, 3)])
@pytest.mark.parametrize("cname", CONFIGS)
def test_want_heads_adds_one_launch_per_layer_and_chunk(cname, chunk, n_chunks):
    attrs = dict(prefill_chunk=chunk)
    plain, _, c = _log(cname, attrs=attrs)
    log, res, _ = _log(cname, attrs=attrs, want_heads=True)
    hr = _head_rows(log)
    assert len(hr) == c.n_layers * n_chunks
    assert all("capture=T" in l and "heads=None" in l and "vec=None" in l and f"n_heads={c.n_heads}, head_dim={c.head_dim}" in l for l in hr)
    assert _names(log, drop=("head_rows",)) == _names(plain) + ["torch.clone"]       # ... and the copy of the result, nothing else
    assert tuple(res.head_out.shape) == (5, c.n_layers, c.n_heads, c.head_dim) and res.head_out.dtype == torch.bfloat16
    # every launch follows its layer's attention (and nothing sits between it and the o GEMM but a knockout's rewrite, absent here)
    names = _names(log)
    for i, n in enumerate(names):
        if n == "head_rows":
            assert names[i - 1] == "attn_fwd" and names[i + 1] in ("gemm", "gemm_rmsnorm"), names[i - 1:i + 2]


@pytest.mark.parametrize("cname", CONFIGS)
def test_a_patch_launches_only_in_its_layers_and_in_chunks_that_list_a_row(cname):
    attrs = dict(prefill_chunk=2)
    plain, _, c = _log(cname, attrs=attrs)
    log, _, _ = _log(cname, attrs=attrs, head_patch=_hp([(1, 2), (1, 0)], rows=[3, 0]))
    hr = _head_rows(log)
    # layer 1 only; chunk (5, 9) lists prompt 0, chunk (7, 4) prompt 3, chunk (6,) none.  7b_lora trims its last layer: gathered rows
    rows = ["rows=i32[0]", "rows=i32[1]"] if cname == "7b_lora" else ["rows=i32[4]", "rows=i32[10]"]
    assert len(hr) == 2 and [r in l for r, l in zip(rows, hr)] == [True, True], hr
    assert all("capture=None" in l and "mode='replace'" in l and "alpha=1.0" in l for l in hr)
    assert _but_for_the_patch(log) == _names(plain)
    # with a capture of all next to it: a capture launch in every layer and chunk, and the two patch launches after theirs
    both, _, _ = _log(cname, attrs=attrs, want_heads=True, head_patch=_hp([(1, 2), (1, 0)], rows=[3, 0]))
    kinds = ["cap" if "capture=T" in l else "patch" for l in _head_rows(both)]
    assert kinds == ["cap", "cap", "patch", "cap", "cap", "patch", "cap", "cap"]       # chunk by chunk, layer 0 then layer 1
    # a patch of every sequence and a capture: one launch does both, in the patched layer
    one, _, _ = _log(cname, want_heads=True, head_patch=_hp([(1, 2), (1, 0)]))
    assert [("capture=T" in l, "vec=T" in l) for l in _head_rows(one)] == [(True, False), (True, True)]


@pytest.mark.parametrize("cname", CONFIGS)
def test_steps_all_adds_one_launch_per_patched_layer_and_step(cname):
    plain, _, c = _log(cname)
    log, _, _ = _log(cname, head_patch=_hp([(1, 2), (0, 1), (1, 0)], rows=[0, 3], steps="all", mode="add", alpha=0.5))
    hr = _head_rows(log)
    assert len(hr) == 2 * (1 + 3)                            # two layers hold a selected head: the prefill and three decode steps
    assert _but_for_the_patch(log) == _names(plain)          # the decode step keeps its form: no launch of another kind
    assert all("mode='add'" in l and "alpha=0.5" in l for l in hr)
    # layer 0 holds one pair, layer 1 two: the head list and the vectors are slices of the sorted buffers
    assert ["[1]/" in l.split(", heads=")[1].split(",")[0] for l in hr] == [True, False] * 4
    prompt_only, _, _ = _log(cname, head_patch=_hp([(1, 2), (0, 1), (1, 0)], rows=[0, 3]))
    assert len(_head_rows(prompt_only)) == 2


@pytest.mark.parametrize("cname", CONFIGS[:2])
def test_overlong_drop_hands_the_survivors_vectors_on(cname):
    log, res, c = _log(cname, lens=lt._overlong_third, overlong="drop", want_heads=True,
                       head_patch=_hp([(1, 2)], rows=[2, 3], fill=[0.0, 1.0, 2.0, 3.0, 4.0]))
    assert res.dropped == (2,) and tuple(res.head_out.shape) == (5, c.n_layers, c.n_heads, c.head_dim)
    patches = [l for l in _head_rows(log) if "vec=T" in l]
    assert len(patches) == 1 and "rows=i32[17]" in patches[0]          # prompt 3, the third of the survivors (5 + 9 + 4 rows)
    vals = []
    for l in log:
        m = re.search(r"host:float32(\[[^a-zA-Z]*\])", l) if l.startswith("torch.copy_(") else None
        if m:
            vals.append(torch.tensor(ast.literal_eval(m.group(1))))
    vec = [v for v in vals if v.dim() == 3]
    assert len(vec) == 1 and tuple(vec[0].shape) == (1, 1, c.head_dim) and bool((vec[0] == 3.0).all())


# ---- graph keys -----------------------------------------------------------------------------------------------------------
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


def test_graph_keys_of_a_head_patch(monkeypatch):
    """What keys a decode graph with a head patch of every step: its uid — listed rows, shared or per-row vectors, the layers that
    launch with their head counts, mode, steps, alpha — appended to the key of the plain call; not the vectors, the rows or the
    head indices, which live in buffers refilled on every call."""
    fake = FakeGraphs(monkeypatch)
    with _traced("tiny_h4", use_graphs=True) as (rt, rec):
        rt._graph_reset()
        c = rt.lm_cfg

        def run(**kw):
            """(replays, graphs kept) after one call"""
            r = fake.replays
            rt.generate(lt.prompts_of(), None, max_new_tokens=3, **kw)
            return fake.replays - r, len(rt._graphs)

        def hp(pairs, rows=(0, 3), steps="all", fill=0.0, mode="add", alpha=0.5, shared=False):
            return dict(heads=pairs, vectors=torch.full((1 if shared else 5, len(pairs), c.head_dim), fill), mode=mode, alpha=alpha,
                        steps=steps, rows=list(rows))

        assert [run() for _ in range(2)] == [(0, 0), (1, 1)]
        (plain,) = rt._graphs
        assert plain == (5, 64, 2, c.eos_id, c.pad_id, None, False, "bf16")
        assert [run(head_patch=hp([(1, 2), (0, 1)])) for _ in range(2)] == [(0, 1), (1, 2)]
        assert list(rt._graphs)[1] == plain + (("head_patch", 2, 2, ((0, 1), (1, 1)), "add", "all", 0.5),)
        # other vectors, other rows and other head indices of the same per-layer counts replay
        assert run(head_patch=hp([(0, 3), (1, 0)], rows=(4, 1), fill=1.0)) == (1, 2)
        # another alpha, another mode, other counts (per layer, of rows, of vector blocks) capture anew
        assert [run(head_patch=hp([(1, 2), (0, 1)], alpha=0.25)) for _ in range(2)] == [(0, 2), (1, 3)]
        assert [run(head_patch=hp([(1, 2), (0, 1)], mode="replace")) for _ in range(2)] == [(0, 3), (1, 4)]
        assert [run(head_patch=hp([(1, 2), (1, 1)])) for _ in range(2)] == [(0, 4), (1, 5)]
        assert [run(head_patch=hp([(1, 2), (0, 1)], rows=(0,))) for _ in range(2)] == [(0, 5), (1, 6)]
        assert [run(head_patch=hp([(1, 2), (0, 1)], shared=True)) for _ in range(2)] == [(0, 6), (1, 7)]
        # a capture and a prompt-only patch leave the decode steps the plain ones
        assert run(want_heads=True) == (1, 7) and run(head_patch=hp([(1, 2)], steps="prompt")) == (1, 7)
        assert [k[:8] for k in rt._graphs] == [plain] * 7

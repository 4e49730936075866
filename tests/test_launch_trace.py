"""The launches of the Llama decoder runtime are pinned (no GPU needed): LlamaHIP.prefill / decode_step / logits make the same
library calls, with the same operands, in the same order as when tests/golden/llama_launch_trace.json was written — at real
7B dims, a grouped-query and a head_dim-64 decoder, both weight modes, both KV dtypes, every switch and every batch-size
boundary (tests/tools/launch_trace.py has the matrix and the encoding).  A change to runtime/engines.py that is meant to keep
behaviour keeps these digests; one that is meant to change a launch regenerates the fixture on purpose
(`python tests/tools/launch_trace.py --write`) and says so.

The generation driver above them (runtime/salmonn.py: generate / _generate_beam) is pinned the same way, one digest per case in
tests/golden/generate_launch_trace.json: launches, the torch plumbing between them, the phase marks and the result's shape.  Its
HIP-graph protocol cannot run on ``meta`` tensors and is covered with fakes at the end of this file."""
import contextlib
import gc
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import launch_trace as lt  # noqa: E402


@pytest.fixture(scope="module")
def got():
    if not lt.device_ok():
        pytest.skip(f"the fixture is taken at {lt.N_CU} CUs (MI355X); this device has another count")
    return lt.digests()


def test_matrix_shape():
    """Under 100 groups; the FP8 KV cache is never paired with the grouped-query config."""
    gs = list(lt.groups())
    assert len(gs) == len(set(gs)) == 84
    assert not [g for g in gs if g[0] == "7b_gqa8_bias" and g[2] == "fp8"]
    assert set(lt.load_fixture()) == {"/".join(g) for g in gs}


def test_launch_trace_matches_the_fixture(got):
    want = lt.load_fixture()
    bad = sorted(k for k in want if got.get(k) != want[k])
    assert not bad, f"{len(bad)} of {len(want)} groups launch differently (diff two `launch_trace.py --dump` runs): {bad[:8]}"
    assert set(got) == set(want)


def test_trace_sees_the_routes(got):
    """The digests are not blind: every switch changes its config's trace, as do the weight mode and the KV dtype."""
    for cname in ("7b_lora", "tiny_h4"):
        base = got[f"{cname}/bf16/bf16/default"]
        for sw in lt.SWITCHES:
            if sw == "default" or (cname == "tiny_h4" and sw in ("no_prefill_last_rows", "no_decode_t256")):
                continue        # head_dim 64 never trims the last layer; its GEMMs are too small for the 256 tile's split
            assert got[f"{cname}/bf16/bf16/{sw}"] != base, (cname, sw)
        assert got[f"{cname}/fp8/bf16/default"] != base and got[f"{cname}/bf16/fp8/default"] != base


# ---- the generation driver -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gen_got():
    if not lt.device_ok():
        pytest.skip(f"the fixture is taken at {lt.N_CU} CUs (MI355X); this device has another count")
    return lt.generate_digests()


def test_generate_matrix_shape():
    cases = ["/".join(c) for c in lt.GEN_MATRIX]
    assert len(cases) == len(set(cases)) == 101
    assert set(lt.load_fixture(lt.GEN_FIXTURE)) == set(cases)


def test_generate_trace_matches_the_fixture(gen_got):
    want = lt.load_fixture(lt.GEN_FIXTURE)
    bad = sorted(k for k in want if gen_got.get(k) != want[k])
    assert not bad, f"{len(bad)} of {len(want)} generate cases differ (diff two `launch_trace.py --dump` runs): {bad}"
    assert set(gen_got) == set(want)


def test_generate_trace_sees_the_modes(gen_got):
    """Not blind: greedy, chunked, sampled, penalised, constrained and beam search differ pairwise; one chunk is no chunking."""
    names = ("greedy4", "chunk2", "sample_seeded", "repetition_penalty", "constrained", "beam3")
    assert len({gen_got[f"tiny_h4/bf16/{n}"] for n in names}) == len(names)
    assert gen_got["tiny_h4/bf16/chunk5"] == gen_got["tiny_h4/bf16/greedy4"]
    # ... and so do the probes: plain, readout, knockout, the residual and the head captures and patches, and cuts, on every
    # config that runs them
    probes = ("greedy4", "prompt_attention", "knockout", "hidden", "patch_all_steps", "heads", "head_patch_all_steps",
              "heads_patch_shared", "cuts")
    for cname in ("tiny_h4", "7b_gqa8_bias"):
        assert len({gen_got[f"{cname}/bf16/{n}"] for n in probes}) == len(probes), cname
    assert len({gen_got[f"7b_lora/bf16/{n}"] for n in probes[1:]}) == len(probes) - 1
    drops = ("drop_knockout", "drop_hidden_patch", "drop_cuts", "drop_head_patch")
    for cname in ("tiny_h4", "7b_lora", "7b_gqa8_bias"):
        assert len({gen_got[f"{cname}/bf16/{n}"] for n in drops}) == len(drops), cname


@pytest.fixture
def traced():
    """(runtime on ``meta``, recorder), recording for the length of the test."""
    if not lt.device_ok():
        pytest.skip(f"the trace is taken at {lt.N_CU} CUs (MI355X); this device has another count")
    rec = lt.Recorder()
    with lt.generate_recording(rec):
        yield lt.generate_runtime("7b_gqa8_bias", "bf16", rec), rec


@pytest.mark.parametrize("kw", [dict(do_sample=True, top_k=2000), dict(repetition_penalty=0), dict(do_sample=True, top_p=0.0),
                                dict(do_sample=True, temperature=0.0)], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_sampling_knobs_are_refused_before_any_launch(traced, kw):
    rt, rec = traced
    with pytest.raises(ValueError, match="top_k" if "top_k" in kw else "sampling knobs"):
        rt.generate(lt.prompts_of(), None, max_new_tokens=4, **kw)
    assert rec.log == [] and rec.requests == {}


# ---- the HIP-graph protocol of generate(), with stand-ins for the graph API --------------------------------------------------------
class FakeGraphs:
    """torch.cuda.CUDAGraph / torch.cuda.graph / torch.cuda.synchronize: ``graph`` runs its body once and notes what
    binding.GEMM_PROFILE was inside and whether the garbage collector was on; a graph object counts its replays."""

    def __init__(self, monkeypatch, B):
        self.replays, self.profile_inside, self.gc_inside = 0, [], []
        outer = self

        class Graph:
            def replay(self):
                outer.replays += 1

        @contextlib.contextmanager
        def graph(g):
            assert isinstance(g, Graph)
            outer.profile_inside.append(B.GEMM_PROFILE)
            outer.gc_inside.append(gc.isenabled())
            yield
        monkeypatch.setattr(torch.cuda, "CUDAGraph", Graph)
        monkeypatch.setattr(torch.cuda, "graph", graph)
        monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)


def test_graph_protocol_eager_capture_replay(monkeypatch):
    if not lt.device_ok():
        pytest.skip(f"the trace is taken at {lt.N_CU} CUs (MI355X); this device has another count")
    B = lt._modules()[0]
    rec = lt.Recorder()
    fake = FakeGraphs(monkeypatch, B)
    profile = object()
    monkeypatch.setattr(B, "GEMM_PROFILE", profile)
    with lt.generate_recording(rec):
        rt = lt.generate_runtime("tiny_h4", "bf16", rec)
        rt.phase_marks, rt.use_graphs = None, True
        rt._graph_reset()
        real_step, calls, failing = rt.llama.decode_step, [], []

        def decode_step(*a, **kw):
            calls.append(1)
            if failing:
                raise RuntimeError("inside the capture")
            return real_step(*a, **kw)
        rt.llama.decode_step = decode_step

        def run(**kw):
            """(decode steps, replays) of one call"""
            n, r = len(calls), fake.replays
            rt.generate(lt.prompts_of(), None, **{"max_new_tokens": 3, **kw})
            return len(calls) - n, fake.replays - r

        assert [run() for _ in range(2)] == [(2, 0), (2, 1)]                 # eager; capture + replay
        assert len(rt._graphs) == 1 and fake.profile_inside == [None] and B.GEMM_PROFILE is profile
        assert fake.gc_inside == [False] and gc.isenabled()                  # no finaliser of a dead cycle runs inside a capture
        assert [run() for _ in range(2)] == [(0, 1), (0, 1)]                 # replay; replay
        (key,) = rt._graphs
        assert key[5] is None                                                # greedy
        rt.ws.release("gen_pos")                                             # a workspace move retires the graphs
        assert run() == (2, 0) and rt._graphs == {}
        assert run() == (2, 1) and run() == (0, 1)
        # a sampled loop is captured under its own key
        assert [run(do_sample=True, top_k=5) for _ in range(2)] == [(2, 0), (2, 1)]
        assert sorted(k[5] is not None for k in rt._graphs) == [False, True]
        # the body raises inside the capture: the profile is restored, nothing is kept
        run(max_new_tokens=2)
        failing.append(True)
        with pytest.raises(RuntimeError, match="inside the capture"):
            run(max_new_tokens=2)
        failing.clear()
        assert fake.profile_inside[-1] is None and B.GEMM_PROFILE is profile and len(rt._graphs) == 2
        assert fake.gc_inside[-1] is False and gc.isenabled()
        # MAX_GRAPHS + 1 keys (the largest first, so that no buffer grows and retires them): the oldest goes
        rt._graph_reset()
        lengths = list(range(rt.MAX_GRAPHS + 2, 1, -1))
        for T in lengths:
            assert [run(max_new_tokens=T) for _ in range(2)] == [(T - 1, 0), (T - 1, 1)]
        assert [k[2] for k in rt._graphs] == [T - 1 for T in lengths[1:]]


def test_graph_keys_of_the_probes(monkeypatch):
    """What keys a decode graph with a probe: a knockout's shape (listed rows, layer window) and a ``steps="all"`` patch's uid,
    appended to the key of the plain call — not the blocked sets or the vectors, which live in buffers refilled on every call."""
    if not lt.device_ok():
        pytest.skip(f"the trace is taken at {lt.N_CU} CUs (MI355X); this device has another count")
    rec = lt.Recorder()
    fake = FakeGraphs(monkeypatch, lt._modules()[0])
    with lt.generate_recording(rec):
        rt = lt.generate_runtime("tiny_h4", "bf16", rec)
        rt.phase_marks, rt.use_graphs = None, True
        rt._graph_reset()
        c, segs = rt.lm_cfg, lt.segments_of(lt.GEN_LENS)

        def run(**kw):
            """(replays, graphs kept) after one call"""
            r = fake.replays
            rt.generate(lt.prompts_of(), None, max_new_tokens=3, **kw)
            return fake.replays - r, len(rt._graphs)

        def patch(site, steps="all", fill=0.0):
            return dict(site=site, vectors=torch.full((5, c.hidden), fill), mode="add", alpha=0.5, steps=steps, rows=[0, 3])

        assert [run() for _ in range(2)] == [(0, 0), (1, 1)]
        (plain,) = rt._graphs
        assert plain == (5, 64, 2, c.eos_id, c.pad_id, None, False, "bf16")        # without probes: today's key, element for element
        blocked = [[1], [], [], [0, 2], []]
        assert [run(knockout=(segs, blocked, (1, 2), [1, 3])) for _ in range(2)] == [(0, 1), (1, 2)]
        # the same shape with other blocked sets and heads: the same uid over refilled buffers replays
        assert run(knockout=(segs, [[2], [], [], [1], []], (1, 2), None)) == (1, 2)
        assert list(rt._graphs)[1] == plain + (("knockout", 2, 1, 2),)
        # another layer window, another number of listed rows: graphs of their own
        assert [run(knockout=(segs, blocked, (0, 2), [1, 3])) for _ in range(2)] == [(0, 2), (1, 3)]
        assert [run(knockout=(segs, [[1], [], [], [], []], (1, 2))) for _ in range(2)] == [(0, 3), (1, 4)]
        # a patch of every step keys by its uid: other vectors replay, another site captures
        assert [run(patch=patch(1)) for _ in range(2)] == [(0, 4), (1, 5)]
        assert run(patch=patch(1, fill=1.0)) == (1, 5)
        assert list(rt._graphs)[4] == plain + (("resid_patch", 2, 2, 1, "add", "all", 0.5),)
        assert [run(patch=patch(0)) for _ in range(2)] == [(0, 5), (1, 6)]
        # a prompt-only patch and a capture leave the decode steps the plain ones
        assert run(patch=patch(1, steps="prompt")) == (1, 6) and run(want_hidden=True) == (1, 6)
        assert [k[:8] for k in rt._graphs] == [plain] * 6

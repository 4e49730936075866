"""Residual-stream capture and patching, without a GPU: the float64 reference and the assertions of tests/resid_patch_ref.py admit
an f32 emulation of icl_resid_rows_f32 on every launch of the table and reject six one-mistake mutants on every launch that could
show the mistake; the far-offset case keeps every 32-bit narrowing inside the arena and inside a compared window; and
``generate(patch=...)`` refuses what it must before anything is sized or launched (runtimes without a device: a launch would be an
AttributeError, not the ValueError asserted)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import far_layout as fl
import resid_patch_ref as rr

SHAPES = [(h, n) for h in rr.HIDDENS for n in rr.N_ROWS]
IDS = [f"h{h}-n{n}" for h, n in SHAPES]


def test_fma32_is_one_rounding_of_the_exact_value():
    """``fma32`` against exact rational arithmetic, on values chosen to sit near rounding ties and on the cancellation probe."""
    g = np.random.default_rng(5)
    a = g.standard_normal(4000).astype(np.float32)
    v = g.standard_normal(4000).astype(np.float32)
    h = g.standard_normal(4000).astype(np.float32) * np.float32(2.0) ** g.integers(-30, 30, 4000).astype(np.float32)
    h[:1000] = -(a[:1000].astype(np.float64) * v[:1000].astype(np.float64)).astype(np.float32)         # cancellation
    h[1000:1500] = np.float32(2.0 ** 24) * np.sign(h[1000:1500])                                       # sums next to a tie
    got = rr.fma32(a, v, h)
    for i in range(len(a)):
        x = Fraction(float(a[i])) * Fraction(float(v[i])) + Fraction(float(h[i]))
        # the two f32 neighbours of x around fl32(float(x)); float(x) is correctly rounded to f64, which orders them correctly
        c = np.float32(float(x))
        cands = {float(c), float(np.nextafter(c, np.float32(np.inf))), float(np.nextafter(c, np.float32(-np.inf)))}
        best = min(abs(Fraction(y) - x) for y in cands)
        ties = [y for y in cands if abs(Fraction(y) - x) == best]
        want = ties[0] if len(ties) == 1 else next(y for y in ties if (np.float32(y).view(np.uint32) & 1) == 0)
        assert float(got[i]) == want, (i, float(a[i]), float(v[i]), float(h[i]))
    assert (got[:1000] != 0).sum() > 500            # the probe leaves the product's rounding error, mostly non-zero


@pytest.mark.parametrize("hidden,n_rows", SHAPES, ids=IDS)
def test_the_emulation_passes_and_every_mutant_is_rejected(hidden, n_rows):
    tried = {m: 0 for m in rr.MUTANTS}
    for c in rr.launch_cases(hidden, n_rows):
        h, rows, vec = rr.inputs(c)
        e = rr.expect(c, h, rows, vec)
        fails, worst = rr.check(c, e, *rr.emulate(c, h, rows, vec))
        assert not fails and worst <= 1.0, (c.id, fails, worst)
        for m in rr.MUTANTS:
            if rr.mutant_applies(m, c):
                tried[m] += 1
                fails, _ = rr.check(c, e, *rr.emulate(c, h, rows, vec, mutant=m))
                assert fails, f"{c.id}: mutant {m} passes"
    assert all(n > 0 for m, n in tried.items() if n_rows > 1 or m not in ("next_vector", "shared_vector")), tried


@pytest.mark.parametrize("hidden,n_rows", [(1028, 3), (4, 65)])
def test_the_cancellation_probe_separates_fused_from_multiply_then_add(hidden, n_rows):
    c = rr.Launch(hidden, n_rows, False, "add", False, "cancel", 0.7)
    h, rows, vec = rr.inputs(c)
    fused, _ = rr.emulate(c, h, rows, vec)
    split, _ = rr.emulate(c, h, rows, vec, mutant="mul_then_add")
    assert (split[rows, :hidden] == 0).all() and (fused[rows, :hidden] != 0).mean() > 0.5
    assert np.array_equal(fused[rows, :hidden].astype(np.float64), rr.expect(c, h, rows, vec).add_ref)       # the exact residual


@pytest.mark.parametrize("mode", ["replace", "add"])
def test_a_list_and_its_reverse_give_the_same_bits(mode):
    base = rr.Launch(1028, 65, True, mode, False, "bits" if mode == "replace" else "normal", 0.7)
    outs = []
    for c in (base, rr.Launch(**{**base.__dict__, "reverse": True})):
        h, rows, vec = rr.inputs(c)
        out, cap = rr.emulate(c, h, rows, vec)
        outs.append((h, rows, out, cap))
    (h0, r0, o0, c0), (h1, r1, o1, c1) = outs
    assert np.array_equal(h0.view(np.uint32), h1.view(np.uint32)) and np.array_equal(r0, r1[::-1])
    assert np.array_equal(o0.view(np.uint32), o1.view(np.uint32)) and np.array_equal(c0.view(np.uint32), c1[::-1].view(np.uint32))


# ---- the far-offset case ------------------------------------------------------------------------------------------------
def test_far_case_every_narrowing_lands_inside_the_arena_and_a_compared_window():
    case = rr.far_case()
    assert case.op("h").is_far() and case.op("h").meta["ld"] == fl.LD_FAR == 2 ** 32 + 64
    wins = sorted((o.base + lo, o.base + hi, o.name) for o in case.ops for lo, hi in o.windows())
    for (lo0, hi0, n0), (lo1, hi1, n1) in zip(wins, wins[1:]):
        assert hi0 <= lo1, f"windows of {n0} and {n1} overlap"
    for o in case.ops:
        assert o.base >= fl.MARGIN and o.base % 256 == 0
        nb = o.n * o.esize
        for off, tw in zip(o.offs, o.twin):
            assert (off * o.esize) % 128 == (tw * o.esize) % 128
            for kind in (None,) + fl.NARROWINGS:
                lo = fl.narrow(off, o.esize, kind)
                assert fl.narrow(off + o.n - 1, o.esize, kind) == lo + nb - o.esize, "a row straddles a 32-bit wrap"
                assert 0 <= o.base + lo - fl.MARGIN and o.base + lo + nb + fl.MARGIN <= fl.ARENA_BYTES, (o.name, off, kind)
                assert any(w0 + fl.MARGIN <= lo and lo + nb <= w1 - fl.MARGIN for w0, w1 in o.windows()), (o.name, off, kind)
        if "ld" in o.meta:
            assert o.meta["ld"] % 4 == 0 and o.meta["ld_twin"] % 4 == 0 and o.meta["ld_twin"] >= o.n
    # a narrowed leading dimension puts row 1 of h 64 elements after row 0: inside row 0's window, where the twin comparison sees it
    h = case.op("h")
    assert {fl.narrow(h.offs[1], 4, k) for k in fl.NARROWINGS} == {64 * 4}


# ---- host validation ----------------------------------------------------------------------------------------------------
def _runtimes():
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.qwen import QwenAudioRuntime
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    cfg = SalmonnCfg.tiny().llama
    for cls in (SalmonnRuntime, QwenAudioRuntime):
        rt = object.__new__(cls)            # no weights, no workspace, no device: anything past the validation raises AttributeError
        rt.lm_cfg, rt.llama, rt.ws, rt.device = cfg, None, None, torch.device("cpu")
        yield rt


@pytest.mark.parametrize("rt", list(_runtimes()), ids=["salmonn", "qwen-audio"])
def test_generate_refuses_a_bad_patch_before_any_launch(rt):
    c = rt.lm_cfg
    prompts = [[[3, 4, 5]], [[6, 7]], [[8, 9, 10, 11]]]
    vec = torch.zeros(3, c.hidden)
    ok = dict(site=1, vectors=vec)
    gen = lambda patch, **kw: rt.generate(prompts, None, max_new_tokens=2, patch=patch, **kw)
    refusals = {
        "unknown": dict(ok, layer=1),
        "dict": ("site", 1),
        "'site' and 'vectors'": dict(vectors=vec),
        f"0..{c.n_layers}": [dict(ok, site=-1), dict(ok, site=c.n_layers + 1), dict(ok, site=1.0), dict(ok, site=True)],
        "float32": [dict(ok, vectors=vec.double()), dict(ok, vectors=vec.to(torch.bfloat16)), dict(ok, vectors=[0.0] * c.hidden)],
        "shape": [dict(ok, vectors=torch.zeros(2, c.hidden)), dict(ok, vectors=torch.zeros(3, c.hidden + 4)),
                  dict(ok, vectors=torch.zeros(1, 3, c.hidden)), dict(ok, vectors=torch.zeros(c.hidden + 4))],
        "mode": [dict(ok, mode="mul"), dict(ok, mode=0)],
        "steps": [dict(ok, steps="decode"), dict(ok, steps=None)],
        "alpha": [dict(ok, mode="add", alpha=float("nan")), dict(ok, mode="add", alpha=float("inf")), dict(ok, alpha="x")],
        "twice": dict(ok, rows=[0, 2, 0]),
        "outside": [dict(ok, rows=[0, 3]), dict(ok, rows=[-1])],
        "rows must be": dict(ok, rows=1),
    }
    for word, patches in refusals.items():
        for patch in (patches if isinstance(patches, list) else [patches]):
            with pytest.raises(ValueError, match=word):
                gen(patch)
    with pytest.raises(ValueError, match="num_beams"):
        gen(ok, num_beams=2)
    with pytest.raises(ValueError, match="num_beams"):
        rt.generate(prompts, None, max_new_tokens=2, want_hidden=True, num_beams=2)
    with pytest.raises(ValueError, match="knockout"):
        gen(ok, knockout=([[0] * 3, [0, 1], [0] * 4], [[], [1], []]))
    with pytest.raises(AttributeError):         # a good patch, and an empty row list (no patch), pass the validation: the first launch
        gen(dict(ok, rows=[2, 0], mode="add", alpha=0.5, steps="all"))
    with pytest.raises(AttributeError):
        gen(dict(ok, rows=[]))
    with pytest.raises(ValueError, match="hidden must be"):
        rt.layer_logits(torch.zeros(3, c.n_layers, c.hidden))

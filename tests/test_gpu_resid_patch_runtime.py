"""`-m gpu`: ``generate(want_hidden=..., patch=...)`` and ``layer_logits`` of the runtime, then the plugin (the launch itself:
tests/test_gpu_resid_patch.py).

3-layer decoders of hidden 512 (tests/probe_harness.py ``Decoder``: a first, a middle and a last layer — trimmed to the last rows in
the multi-head form; grouped 4 / 2 with QK-norm as the second form), five ragged prompts, one with a speech segment, four new tokens.

Exact (bits): ``want_hidden`` changes nothing else; replacing a site by its own captured rows is the unpatched run, at every site
and with the FP8 KV cache; a transplant of another batch's last site gives that batch's first logits; ``layer_logits`` at the last
site is ``first_logits``; prefill chunks, captured decode graphs against eager calls, the unlisted rows of a mixed batch (so the
decode step's fused and separate input norm agree bit for bit on the rows they both compute) and ``overlong="drop"``.

Against transformers in fp32 on the CPU (``output_hidden_states`` read by forward pre-hooks on the decoder layers and on
``model.norm``, the same hooks patching; teacher-forced along the GPU's tokens): rel-L2 of ``hidden`` and of ``layer_logits`` per
site, and of the patched logits per step, next to the same model in bf16 against itself in fp32 — allowed 1.25 x that figure, the
project's criterion; a patch must move HF's own logits by more than 4 x the bf16 error.  Tokens are compared at decisions whose
fp32 margin exceeds 2.5 x the bf16 logit error.  The figures are printed; README.md records them.
"""
from functools import lru_cache

import pytest
import torch

import probe_harness as ph
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)
from probe_harness import PARITY_RATIO, rel as _rel, same_result as _same

pytestmark = pytest.mark.gpu

NEW, L = ph.NEW, 3                                    # a first, a middle and a (trimmed, for the multi-head form) last layer
FORMS = {"mha": (None, False), "gqa-qknorm": (2, True)}
KW = dict(max_new_tokens=NEW, suppress_eos=True, want_first_logits=True, want_step_logits=True)


class _Env(ph.Decoder):
    def __init__(self, kv, qk_norm):
        super().__init__(kv, qk_norm, n_layers=L, other=True)
        self.rt = self.runtime(DEV)
        self.sp = self.speech.to(DEV)
        self.plain = self.rt.generate(self.prompts, self.sp, **KW)
        self.cap = self.rt.generate(self.prompts, self.sp, want_hidden=True, **KW)
        g = torch.Generator().manual_seed(23)
        rms = float(self.cap.hidden[:, 1].float().pow(2).mean().sqrt())
        self.vec = torch.randn(5, self.cfg.llama.hidden, generator=g) * rms        # per-row vectors at the scale of the middle site

    def gen(self, patch=None, prompts=None, **kw):
        return self.rt.generate(self.prompts if prompts is None else prompts, self.sp, **dict(KW, **kw),
                                **({} if patch is None else {"patch": patch}))


@pytest.fixture(scope="module", params=list(FORMS), ids=list(FORMS))
def env(request):
    return _Env(*FORMS[request.param])


def test_want_hidden_changes_nothing_and_the_last_site_is_the_first_logits(env):
    c = env.cfg.llama
    assert env.plain.hidden is None and env.cap.hidden.shape == (5, L + 1, c.hidden) and env.cap.hidden.dtype == torch.float32
    assert _same(env.cap, env.plain)
    lens = env.rt.layer_logits(env.cap.hidden)
    assert lens.shape == (5, L + 1, c.vocab) and torch.equal(lens[:, L], env.plain.first_logits)
    assert bool(torch.isfinite(env.cap.hidden).all())
    for site in range(L):
        assert not torch.equal(env.cap.hidden[:, site], env.cap.hidden[:, site + 1])


def test_identity_replacing_a_site_by_its_own_rows(env):
    for site in range(L + 1):
        res = env.gen(dict(site=site, vectors=env.cap.hidden[:, site].clone()))
        assert _same(res, env.plain), site
        res = env.gen(dict(site=site, vectors=env.cap.hidden[:, site].cpu(), rows=[3, 0]), want_hidden=True)     # a CPU tensor, a subset
        assert _same(res, env.plain) and torch.equal(res.hidden, env.cap.hidden), site
    if env.cfg.llama.group == 1 and not env.cfg.llama.qk_norm:                   # the FP8 KV cache exists for this form only
        rt8 = env.runtime(DEV, llm_kv_dtype="fp8")
        plain = rt8.generate(env.prompts, env.sp, want_hidden=True, **KW)
        assert _same(plain, rt8.generate(env.prompts, env.sp, **KW))
        for site in range(L + 1):
            res = rt8.generate(env.prompts, env.sp, patch=dict(site=site, vectors=plain.hidden[:, site]), **KW)
            assert _same(res, plain), site


def test_transplant_of_the_last_site_gives_the_donor_s_first_logits(env):
    donor = env.gen(prompts=env.other, want_hidden=True)
    res = env.gen(dict(site=L, vectors=donor.hidden[:, L]))
    assert torch.equal(res.first_logits, donor.first_logits) and not torch.equal(res.first_logits, env.plain.first_logits)
    assert torch.equal(res.tokens[:, 0], donor.tokens[:, 0])
    shared = env.gen(dict(site=L, vectors=donor.hidden[2, L]))                    # one vector for every row
    for b in range(5):
        assert torch.equal(shared.first_logits[b], donor.first_logits[2]), b


PATCHES = {
    "replace-mid-prompt": dict(site=1, mode="replace", steps="prompt"),
    "add-mid-all": dict(site=1, mode="add", alpha=0.5, steps="all"),
    "add-last-all-subset": dict(site=L, mode="add", alpha=-0.75, steps="all", rows=[4, 1]),
    "replace-first-all-subset": dict(site=0, mode="replace", steps="all", rows=[0, 2, 3]),
}


@pytest.mark.parametrize("name", list(PATCHES))
def test_prefill_chunks_give_the_same_bits(env, name):
    patch = dict(PATCHES[name], vectors=env.vec)
    one = env.gen(patch, want_hidden=True)
    assert not _same(one, env.plain)
    with ph.prefill_chunks(env.rt, 2):
        two = env.gen(patch, want_hidden=True)
    assert _same(one, two) and torch.equal(one.hidden, two.hidden)
    site = patch["site"]
    assert torch.equal(one.hidden[:, :site + 1], env.cap.hidden[:, :site + 1])    # pre-patch at the patched site; nothing before it moves
    rows = patch.get("rows", list(range(5)))
    if site < L:
        for b in range(5):
            assert torch.equal(one.hidden[b, site + 1:], env.cap.hidden[b, site + 1:]) == (b not in rows), b


def test_graph_replays_see_this_call_s_alpha_vectors_and_rows(env):
    g = torch.Generator().manual_seed(31)
    vecs = [env.vec] + [env.vec[torch.randperm(5, generator=g)] * s for s in (0.5, 2.0)]
    calls = [dict(site=1, mode="add", alpha=a, steps="all", vectors=v, rows=r)
             for a, v, r in ((0.5, vecs[0], [1, 3]), (0.25, vecs[1], [1, 3]), (0.25, vecs[2], [0, 4]), (0.25, vecs[0], [2, 4]), (0.5, vecs[1], [0, 1]))]
    calls += [dict(site=2, mode="replace", steps="all", vectors=v) for v in vecs]
    try:
        env.rt.use_graphs = False
        want = [env.gen(p) for p in calls]
    finally:
        del env.rt.use_graphs
    assert env.rt.use_graphs
    for i, p in enumerate(calls):                   # per key: an eager pass, the capture, then replays
        assert _same(env.gen(p), want[i]), i
    assert not _same(want[1], want[2]) and not _same(want[5], want[6])
    assert _same(env.gen(), env.plain)              # and the plain call is still the plain call


@pytest.mark.parametrize("site", range(L + 1))
@pytest.mark.parametrize("mode", ["add", "replace"])
def test_mixed_batch_unlisted_rows_keep_their_bits(env, site, mode):
    """``steps="all"`` on rows 1 and 3: the patched layer of every decode step runs its input norm as a launch of its own, for all
    rows; the rows not listed must come out with the bits the fused norm gives them."""
    listed = [3, 1]
    res = env.gen(dict(site=site, mode=mode, alpha=0.5, steps="all", rows=listed, vectors=env.vec))
    full = env.gen(dict(site=site, mode=mode, alpha=0.5, steps="all", vectors=env.vec))
    for b in range(5):
        if b in listed:
            assert not torch.equal(res.step_logits[:, b], env.plain.step_logits[:, b]), b
            assert torch.equal(res.step_logits[:, b], full.step_logits[:, b]) and torch.equal(res.tokens[b], full.tokens[b]), b
        else:
            assert torch.equal(res.step_logits[:, b], env.plain.step_logits[:, b]) and torch.equal(res.tokens[b], env.plain.tokens[b]), b
    prompt_only = env.gen(dict(site=site, mode=mode, alpha=0.5, steps="prompt", rows=listed, vectors=env.vec))
    assert torch.equal(prompt_only.first_logits, res.first_logits) and not torch.equal(prompt_only.step_logits[1:], res.step_logits[1:])


def test_overlong_drop_hands_the_surviving_rows_vectors_on(env):
    c = env.cfg.llama
    long_row = [[5] * (c.max_pos - 1)]
    vec6 = torch.cat([env.vec[:2], torch.full((1, c.hidden), 7.0), env.vec[2:]])             # the dropped row's vector in the middle
    prompts = env.prompts[:2] + [long_row] + env.prompts[2:]
    res = env.rt.generate(prompts, env.sp, overlong="drop", want_hidden=True,
                          patch=dict(site=1, mode="add", alpha=0.5, steps="all", vectors=vec6, rows=[5, 2, 1]), **KW)
    want = env.gen(dict(site=1, mode="add", alpha=0.5, steps="all", vectors=env.vec, rows=[4, 1]), want_hidden=True)
    keep = [0, 1, 3, 4, 5]
    assert res.dropped == (2,) and torch.equal(res.tokens[keep], want.tokens) and torch.equal(res.step_logits[:, keep], want.step_logits)
    assert torch.equal(res.hidden[keep], want.hidden) and bool(torch.isnan(res.hidden[2]).all())
    only = env.rt.generate(prompts, env.sp, overlong="drop", patch=dict(site=1, vectors=vec6, rows=[2]), **KW)  # only the dropped row listed
    assert torch.equal(only.step_logits[:, keep], env.plain.step_logits)


def test_other_tails_and_refusals(env):
    from icl_speech_text_llm_amd.runtime.constraints import LabelAutomaton
    rt, c = env.rt, env.cfg.llama
    patch = dict(site=1, mode="add", alpha=0.5, steps="all", vectors=env.vec)
    auto = LabelAutomaton([0, 2, 3, 4], [10, 12, 11, c.eos_id], [1, 2, 2, 2], {}, c.vocab, c.eos_id)
    res = rt.generate(env.prompts, env.sp, max_new_tokens=NEW, patch=patch, constraint=(auto, [0] * 5))
    for b in range(5):
        assert [t for t in res.tokens[b].tolist() if t not in (c.eos_id, c.pad_id)] in ([10, 11], [12]), b
    draws = [rt.generate(env.prompts, env.sp, max_new_tokens=NEW, suppress_eos=True, do_sample=True, top_k=5, temperature=0.7,
                         generator=torch.Generator().manual_seed(99), patch=patch).tokens for _ in range(2)]
    assert torch.equal(draws[0], draws[1]) and draws[0].shape == (5, NEW)
    calls = []
    real = rt.llama.prefill
    rt.llama.prefill = lambda *a, **kw: calls.append(1) or real(*a, **kw)
    try:
        before = rt.ws.nbytes()
        for word, kw in {"site": dict(patch=dict(patch, site=L + 1)), "shape": dict(patch=dict(patch, vectors=env.vec[:4])),
                         "twice": dict(patch=dict(patch, rows=[1, 1])), "num_beams": dict(patch=patch, num_beams=2),
                         "knockout": dict(patch=patch, knockout=([[0] * n for n in env.lens], [[]] * 4 + [[1]]))}.items():
            with pytest.raises(ValueError, match=word):
                rt.generate(env.prompts, env.sp, max_new_tokens=2, **kw)
        assert rt.ws.nbytes() == before and not calls
    finally:
        del rt.llama.prefill


# ------------------------------------------------------------------------------------------------------------------
# against transformers
# ------------------------------------------------------------------------------------------------------------------
def _ratio(mine, own):
    return mine / own if own > 0 else (0.0 if mine == 0 else float("inf"))


@lru_cache(maxsize=None)
def _hf_plain(env):
    hf = env.hf()
    return ph.resid_run(env, hf, torch.float32, env.plain.tokens), ph.resid_run(env, hf, torch.bfloat16, env.plain.tokens)


def test_hidden_and_the_logit_lens_against_transformers(env):
    (lg32, hid32, lens32), (lg16, hid16, lens16) = _hf_plain(env)
    hidden = env.cap.hidden.double().cpu()
    lens = env.rt.layer_logits(env.cap.hidden).double().cpu()
    tag = f"kv={env.cfg.llama.n_kv_heads} qk_norm={env.cfg.llama.qk_norm}"
    for site in range(L + 1):
        for what, got, w32, w16 in (("hidden", hidden, hid32, hid16), ("layer_logits", lens, lens32, lens16)):
            own, mine = _rel(w16[:, site], w32[:, site]), _rel(got[:, site], w32[:, site])
            print(f"{tag} site {site} {what}: rel-L2 vs HF fp32 {mine:.3e}; HF bf16 vs HF fp32 {own:.3e}; ratio {_ratio(mine, own):.3f} "
                  f"(allowed {PARITY_RATIO})")
            assert mine <= PARITY_RATIO * own, (site, what)


@pytest.mark.parametrize("name", ["replace-mid-prompt", "add-mid-all"])
def test_patched_logits_against_transformers(env, name):
    patch = dict(PATCHES[name], vectors=env.vec)
    res = env.gen(patch)
    got = res.step_logits.double().cpu()
    hf = env.hf()
    want32, _, _ = ph.resid_run(env, hf, torch.float32, res.tokens, patch)
    want16, _, _ = ph.resid_run(env, hf, torch.bfloat16, res.tokens, patch)
    free32, _, _ = ph.resid_run(env, hf, torch.float32, res.tokens)
    # (a prompt-only patch reaches the later steps through the cache alone; transformers on the CPU, on its own greedy tokens:
    # 8 x the bf16 error or more at those steps, 55 x or more wherever the patch acts directly; 7 to 16 of the 20 margins decisive)
    ph.parity_check(got, want32, want16, free32, res.tokens, f"{name} kv={env.cfg.llama.n_kv_heads} qk_norm={env.cfg.llama.qk_norm}",
                    effect_floor=4, min_decisive=res.tokens.numel() // 4)


# ------------------------------------------------------------------------------------------------------------------
# the launch trace (on the meta device: nothing runs)
# ------------------------------------------------------------------------------------------------------------------
def test_launch_trace():
    """``want_hidden`` adds one resid_rows launch per site and prefill chunk and nothing else; a ``steps="all"`` patch adds one per
    chunk that lists a row and one per decode step, plus the patched layer's input norm (the final norm at the last site) as a
    launch of its own in every step whose previous ``down`` launch had fused it."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    import launch_trace as lt
    lens = list(lt.GEN_LENS)

    def trace(cname, attrs=None, **kw):
        rec = lt.Recorder()
        rt = lt.generate_runtime(cname, "bf16", rec)
        for k, v in (attrs or {}).items():
            setattr(rt, k, v)
        with lt.generate_recording(rec):
            rt.generate(lt.prompts_of(lens), None, max_new_tokens=4, **kw)
        return [x.split("(")[0] for x in rec.log if "(" in x and not x.startswith("torch.")]

    without = lambda names, *drop: [x for x in names if x not in drop]
    for cname in ("tiny_h4", "7b_gqa8_bias", "7b_nolora"):
        cfg = lt.configs()[cname]
        n_sites = cfg.n_layers + 1
        vec = torch.zeros(len(lens), cfg.hidden)
        for attrs, chunks in (({}, 1), (dict(prefill_chunk=2), 3)):
            base = trace(cname, attrs)
            assert "resid_rows" not in base
            log = trace(cname, attrs, want_hidden=True)
            assert log.count("resid_rows") == n_sites * chunks and without(log, "resid_rows") == base, (cname, attrs)
            for site in range(n_sites):
                # rows 0 and 3: chunks [0, 1] and [2, 3] of the three list a row
                log = trace(cname, attrs, patch=dict(site=site, vectors=vec, mode="add", alpha=0.5, steps="all", rows=[0, 3]))
                listing = 1 if chunks == 1 else 2
                assert log.count("resid_rows") == listing + 3, (cname, attrs, site)
                assert log.count("rmsnorm") - base.count("rmsnorm") == (3 if site > 0 else 0), (cname, attrs, site)
                assert without(log, "resid_rows", "rmsnorm") == without(base, "rmsnorm"), (cname, attrs, site)
                log = trace(cname, attrs, patch=dict(site=site, vectors=vec, steps="prompt", rows=[0, 3]))
                assert log.count("resid_rows") == listing and without(log, "resid_rows") == base, (cname, attrs, site)
                log = trace(cname, attrs, want_hidden=True, patch=dict(site=site, vectors=vec))      # all rows: capture + patch in one
                assert log.count("resid_rows") == n_sites * chunks and without(log, "resid_rows") == base, (cname, attrs, site)


# ------------------------------------------------------------------------------------------------------------------
# the plugin
# ------------------------------------------------------------------------------------------------------------------
def test_plugin():
    model, few, zero = ph.tiny_plugin_batches(2, 0)
    c = model.cfg.llama
    tv = model.task_vectors(dict(few))
    assert set(tv) == {"hidden", "first_logits", "tokens", "texts"} and tv["hidden"].shape == (2, c.n_layers + 1, c.hidden)
    plain_few = model.generate_ids(dict(few), want_first_logits=True)
    assert torch.equal(tv["first_logits"], plain_few.first_logits) and torch.equal(tv["tokens"], plain_few.tokens)
    assert torch.equal(model.runtime.layer_logits(tv["hidden"])[:, c.n_layers], tv["first_logits"])
    site = c.n_layers // 2
    with ph.spy_generate(model) as seen:
        out = model.generate_patched(dict(zero), tv["hidden"][:, site], site)
    assert set(out) == {"texts", "tokens", "first_logits"} and len(out["texts"]) == 2 and out["first_logits"].shape == (2, c.vocab)
    assert seen["kw"]["patch"]["site"] == site and seen["kw"]["patch"]["mode"] == "replace" and seen["kw"]["patch"]["steps"] == "prompt"
    direct = model.runtime.generate(seen["segs"], seen["speech"], **seen["kw"])                 # the runtime-level call
    assert torch.equal(direct.first_logits, out["first_logits"]) and torch.equal(direct.tokens, out["tokens"])
    plain_zero = model.generate_ids(dict(zero), want_first_logits=True)
    assert not torch.equal(out["first_logits"], plain_zero.first_logits)
    last = model.generate_patched(dict(zero), tv["hidden"][:, c.n_layers], c.n_layers)          # the last site: the donor's first logits
    assert torch.equal(last["first_logits"], tv["first_logits"])
    steer = model.generate_patched(dict(zero), tv["hidden"][0, site], site, mode="add", alpha=0.5, steps="all", rows=[1])
    assert torch.equal(steer["first_logits"][0], plain_zero.first_logits[0]) and not torch.equal(steer["first_logits"][1], plain_zero.first_logits[1])
    with pytest.raises(ValueError, match="shape"):
        model.generate_patched(dict(zero), tv["hidden"][:, site, :-4], site)
    with pytest.raises(ValueError, match="shape"):
        model.generate_patched(dict(zero), tv["hidden"], site)
    assert torch.equal(model.generate_ids(dict(zero), want_first_logits=True).first_logits, plain_zero.first_logits)

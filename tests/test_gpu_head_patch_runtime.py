"""`-m gpu`: ``generate(want_heads=..., head_patch=...)`` and ``head_contrib`` of the runtime, then the plugin (the launch itself:
tests/test_gpu_head_rows.py).

The decoders of tests/test_gpu_resid_patch_runtime.py (tests/probe_harness.py ``Decoder``: 3 layers of hidden 512, 4 heads of 128 —
multi-head with the trimmed last layer, and grouped 4 / 2 with QK-norm), five ragged prompts, one with a speech segment, four new
tokens.

Exact (bits): ``want_heads`` changes no token and no logit, also next to a knockout and next to a residual patch; replacing all
heads of a layer by their own captured values is the unpatched run, also with the FP8 KV cache and at 12 rows, where the decode
step fuses RoPE into the attention launch (there an add of 0 x v in every step is the unpatched run too); prefill chunks of two;
captured decode graphs against eager calls; the unlisted rows of a mixed batch in every step; ``overlong="drop"``.

``head_contrib`` per element against float64 on the same bf16 operands within ``gemm_ref_bound`` at K = head_dim, and its sum over
a layer's heads against the same reference of the whole row.

Against transformers in fp32 on the CPU (a forward pre-hook on every layer's ``self_attn.o_proj`` reads and patches its input's
last row; teacher-forced along the GPU's tokens): rel-L2 of ``head_out`` per layer and of the logits per step next to the same
model in bf16 against itself in fp32 — allowed 1.25 x that figure, the project's criterion.  Tokens are compared at decisions
whose fp32 margin exceeds 2.5 x the largest bf16 logit error: at least 8 of the 20.  The figures are printed; README.md records them.
"""
import pytest
import torch

import fp64_bounds as fb
import probe_harness as ph
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)
from probe_harness import PARITY_RATIO, rel as _rel, same_result as _same

pytestmark = pytest.mark.gpu

NEW, L = ph.NEW, 3
FORMS = {"mha": (None, False), "gqa-qknorm": (2, True)}
KW = dict(max_new_tokens=NEW, suppress_eos=True, want_first_logits=True, want_step_logits=True)
ALL = lambda c, layer: [(layer, h) for h in range(c.n_heads)]


class _Env(ph.Decoder):
    def __init__(self, kv, qk_norm):
        super().__init__(kv, qk_norm, n_layers=L, other=True)
        self.rt = self.runtime(DEV)
        self.sp = self.speech.to(DEV)
        self.plain = self.gen()
        self.cap = self.gen(want_heads=True)
        g = torch.Generator().manual_seed(29)
        c = self.cfg.llama
        rms = self.cap.head_out.float().pow(2).mean(dim=(0, 3)).sqrt().cpu()                  # [L, H]: every head's own scale
        self.vec = torch.randn(5, L, c.n_heads, c.head_dim, generator=g) * rms[None, :, :, None]
        self.twelve = self.prompts + self.other + [[torch.randint(3, c.vocab - 1, (n,), generator=g).tolist()] for n in (21, 58)]

    def gen(self, hp=None, prompts=None, rt=None, **kw):
        return (rt or self.rt).generate(self.prompts if prompts is None else prompts, self.sp, **dict(KW, **kw),
                                        **({} if hp is None else {"head_patch": hp}))

    def vectors(self, pairs, rows=slice(None)):
        return torch.stack([self.vec[rows, l, h] for l, h in pairs], dim=1)


@pytest.fixture(scope="module", params=list(FORMS), ids=list(FORMS))
def env(request):
    return _Env(*FORMS[request.param])


def _bits(t):
    return t.contiguous().view(torch.int16)


def test_want_heads_changes_nothing(env):
    c = env.cfg.llama
    assert env.plain.head_out is None and env.cap.head_out.shape == (5, L, c.n_heads, c.head_dim) and env.cap.head_out.dtype == torch.bfloat16
    assert _same(env.cap, env.plain) and bool(torch.isfinite(env.cap.head_out.float()).all())
    for layer in range(L - 1):
        assert not torch.equal(env.cap.head_out[:, layer], env.cap.head_out[:, layer + 1])
    patch = dict(site=1, mode="add", alpha=0.5, steps="all", vectors=torch.randn(5, c.hidden, generator=torch.Generator().manual_seed(3)), rows=[1, 3])
    a, b = env.gen(patch=patch), env.gen(patch=patch, want_heads=True, want_hidden=True)
    assert _same(a, b) and not _same(a, env.plain)
    assert torch.equal(_bits(b.head_out[:, 0]), _bits(env.cap.head_out[:, 0])) and not torch.equal(_bits(b.head_out[:, 1]), _bits(env.cap.head_out[:, 1]))
    ko = ([[j * 4 // n for j in range(n)] for n in env.lens], [[1], [], [], [0, 2], []], (1, 3), [1, 3])
    a, b = env.gen(knockout=ko), env.gen(knockout=ko, want_heads=True)
    assert _same(a, b) and not _same(a, env.plain)
    # the capture is what o_proj reads: after the knockout's rewrite of rows 0 and 3 in layers 1 and 2 (the masked launch writes
    # every head of a listed row, the unmasked ones from the decode kernel's arithmetic: only the masked heads must move)
    assert torch.equal(_bits(b.head_out[:, 0]), _bits(env.cap.head_out[:, 0]))
    for layer in (1, 2):
        for h in (1, 3):
            assert not torch.equal(_bits(b.head_out[[0, 3], layer, h]), _bits(env.cap.head_out[[0, 3], layer, h])), (layer, h)
    assert torch.equal(_bits(b.head_out[[1, 2, 4]]), _bits(env.cap.head_out[[1, 2, 4]]))


def test_identity_replacing_a_layer_s_heads_by_their_own_values(env):
    c = env.cfg.llama
    for layer in range(L):
        own = env.cap.head_out[:, layer].float()
        assert _same(env.gen(dict(heads=ALL(c, layer), vectors=own)), env.plain), layer
        pairs = [(layer, 2), (layer, 0)]                                             # a CPU tensor, a subset of rows and heads, unsorted
        res = env.gen(dict(heads=pairs, vectors=own[:, [2, 0]].cpu(), rows=[3, 0]), want_heads=True)
        assert _same(res, env.plain) and torch.equal(_bits(res.head_out), _bits(env.cap.head_out)), layer
    every = [(l, h) for l in range(L) for h in range(c.n_heads)]
    assert _same(env.gen(dict(heads=every, vectors=env.cap.head_out.float().flatten(1, 2))), env.plain)
    if c.group == 1 and not c.qk_norm:                   # the FP8 KV cache exists for this form only
        rt8 = env.runtime(DEV, llm_kv_dtype="fp8")
        plain = env.gen(rt=rt8, want_heads=True)
        assert _same(plain, env.gen(rt=rt8))
        for layer in range(L):
            assert _same(env.gen(dict(heads=ALL(c, layer), vectors=plain.head_out[:, layer].float()), rt=rt8), plain), layer


def test_twelve_rows_the_fused_rope_decode_step(env):
    c = env.cfg.llama
    plain = env.gen(prompts=env.twelve)
    cap = env.gen(prompts=env.twelve, want_heads=True)
    assert _same(cap, plain)
    g = torch.Generator().manual_seed(41)
    v = torch.randn(12, 2, c.head_dim, generator=g)
    for layer in range(L):
        assert _same(env.gen(dict(heads=ALL(c, layer), vectors=cap.head_out[:, layer].float()), prompts=env.twelve), plain), layer
        # a + 0 x v = a in every step (only a -0.0 would turn into 0.0: not a value the attention produces here)
        zero = env.gen(dict(heads=[(layer, 3), (layer, 1)], vectors=v, mode="add", alpha=0.0, steps="all"), prompts=env.twelve)
        assert _same(zero, plain), layer
        listed = [7, 2, 11]
        res = env.gen(dict(heads=[(layer, 3), (layer, 1)], vectors=v, mode="add", alpha=0.5, steps="all", rows=listed), prompts=env.twelve)
        for b in range(12):
            assert torch.equal(res.step_logits[:, b], plain.step_logits[:, b]) == (b not in listed), (layer, b)


PATCHES = {
    "replace-mid-prompt": dict(heads=[(1, 2), (1, 0)], mode="replace", steps="prompt"),
    "add-two-layers-all": dict(heads=[(2, 1), (0, 3), (2, 0)], mode="add", alpha=0.5, steps="all"),
    "add-last-all-subset": dict(heads=[(L - 1, 3)], mode="add", alpha=-0.75, steps="all", rows=[4, 1]),
    "replace-first-all-subset": dict(heads=[(0, 1), (0, 2)], mode="replace", steps="all", rows=[0, 2, 3]),
}


def _patch(env, name):
    p = dict(PATCHES[name])
    return dict(p, vectors=env.vectors(p["heads"]))


@pytest.mark.parametrize("name", list(PATCHES))
def test_prefill_chunks_give_the_same_bits(env, name):
    hp = _patch(env, name)
    one = env.gen(hp, want_heads=True)
    assert not _same(one, env.plain)
    with ph.prefill_chunks(env.rt, 2):
        two = env.gen(hp, want_heads=True)
    assert _same(one, two) and torch.equal(_bits(one.head_out), _bits(two.head_out))
    first = min(l for l, _ in hp["heads"])
    assert torch.equal(_bits(one.head_out[:, :first + 1]), _bits(env.cap.head_out[:, :first + 1]))   # pre-patch; nothing before it moves
    rows = hp.get("rows", list(range(5)))
    for b in range(5):
        if first + 1 < L:
            assert torch.equal(_bits(one.head_out[b, first + 1:]), _bits(env.cap.head_out[b, first + 1:])) == (b not in rows), b


def test_graph_replays_see_this_call_s_vectors_heads_and_rows(env):
    g = torch.Generator().manual_seed(31)
    vecs = [env.vec] + [env.vec[torch.randperm(5, generator=g)] * s for s in (0.5, 2.0)]
    pick = lambda v, pairs: torch.stack([v[:, l, h] for l, h in pairs], dim=1)
    calls = [dict(heads=p, mode="add", alpha=a, steps="all", vectors=pick(v, p), rows=r)
             for a, v, r, p in ((0.5, vecs[0], [1, 3], [(1, 2), (0, 1)]), (0.5, vecs[1], [1, 3], [(1, 2), (0, 1)]),
                                (0.5, vecs[2], [0, 4], [(0, 3), (1, 0)]), (0.25, vecs[0], [2, 4], [(1, 2), (0, 1)]),
                                (0.5, vecs[1], [0, 1], [(2, 2), (2, 1)]))]
    calls += [dict(heads=[(2, 0), (1, 1), (2, 3)], mode="replace", steps="all", vectors=pick(v, [(2, 0), (1, 1), (2, 3)])) for v in vecs]
    try:
        env.rt.use_graphs = False
        want = [env.gen(p) for p in calls]
    finally:
        del env.rt.use_graphs
    assert env.rt.use_graphs
    for i, p in enumerate(calls):                   # per key: an eager pass, the capture, then replays
        assert _same(env.gen(p), want[i]), i
    assert not _same(want[1], want[2]) and not _same(want[5], want[6]) and not _same(want[0], want[1])
    assert _same(env.gen(), env.plain)              # and the plain call is still the plain call


@pytest.mark.parametrize("layer", range(L))
@pytest.mark.parametrize("mode", ["add", "replace"])
def test_mixed_batch_unlisted_rows_keep_their_bits(env, layer, mode):
    listed, pairs = [3, 1], [(layer, 1), (layer, 2)]
    hp = dict(heads=pairs, mode=mode, alpha=0.5, steps="all", vectors=env.vectors(pairs))
    res, full = env.gen(dict(hp, rows=listed)), env.gen(hp)
    for b in range(5):
        if b in listed:
            assert not torch.equal(res.step_logits[:, b], env.plain.step_logits[:, b]), b
            assert torch.equal(res.step_logits[:, b], full.step_logits[:, b]) and torch.equal(res.tokens[b], full.tokens[b]), b
        else:
            assert torch.equal(res.step_logits[:, b], env.plain.step_logits[:, b]) and torch.equal(res.tokens[b], env.plain.tokens[b]), b
    prompt_only = env.gen(dict(hp, rows=listed, steps="prompt"))
    assert torch.equal(prompt_only.first_logits, res.first_logits) and not torch.equal(prompt_only.step_logits[1:], res.step_logits[1:])


def test_overlong_drop_gives_the_survivors_what_they_get_alone(env):
    c = env.cfg.llama
    pairs = [(1, 2), (0, 1)]
    v5 = env.vectors(pairs)
    v6 = torch.cat([v5[:2], torch.full((1, 2, c.head_dim), 7.0), v5[2:]])                 # the dropped row's vectors in the middle
    prompts = env.prompts[:2] + [[[5] * (c.max_pos - 1)]] + env.prompts[2:]
    hp = dict(heads=pairs, mode="add", alpha=0.5, steps="all")
    res = env.gen(dict(hp, vectors=v6, rows=[5, 2, 1]), prompts=prompts, overlong="drop", want_heads=True)
    want = env.gen(dict(hp, vectors=v5, rows=[4, 1]), want_heads=True)
    keep = [0, 1, 3, 4, 5]
    assert res.dropped == (2,) and torch.equal(res.tokens[keep], want.tokens) and torch.equal(res.step_logits[:, keep], want.step_logits)
    assert torch.equal(_bits(res.head_out[keep]), _bits(want.head_out)) and bool(torch.isnan(res.head_out[2].float()).all())
    only = env.gen(dict(hp, vectors=v6, rows=[2]), prompts=prompts, overlong="drop")       # only the dropped row listed
    assert torch.equal(only.step_logits[:, keep], env.plain.step_logits)


def test_other_tails_and_refusals(env):
    from icl_speech_text_llm_amd.runtime.constraints import LabelAutomaton
    rt, c = env.rt, env.cfg.llama
    hp = _patch(env, "add-two-layers-all")
    auto = LabelAutomaton([0, 2, 3, 4], [10, 12, 11, c.eos_id], [1, 2, 2, 2], {}, c.vocab, c.eos_id)
    res = rt.generate(env.prompts, env.sp, max_new_tokens=NEW, head_patch=hp, constraint=(auto, [0] * 5))
    for b in range(5):
        assert [t for t in res.tokens[b].tolist() if t not in (c.eos_id, c.pad_id)] in ([10, 11], [12]), b
    draws = [rt.generate(env.prompts, env.sp, max_new_tokens=NEW, suppress_eos=True, do_sample=True, top_k=5, temperature=0.7,
                         generator=torch.Generator().manual_seed(99), head_patch=hp).tokens for _ in range(2)]
    assert torch.equal(draws[0], draws[1]) and draws[0].shape == (5, NEW)
    calls = []
    real = rt.llama.prefill
    rt.llama.prefill = lambda *a, **kw: calls.append(1) or real(*a, **kw)
    try:
        before = rt.ws.nbytes()
        for word, kw in {"outside": dict(head_patch=dict(hp, heads=[(L, 0), (0, 1), (0, 2)])), "shape": dict(head_patch=dict(hp, vectors=hp["vectors"][:4])),
                         "twice": dict(head_patch=dict(hp, rows=[1, 1])), "num_beams": dict(head_patch=hp, num_beams=2),
                         "want_heads": dict(want_heads=True, num_beams=2),
                         "with patch": dict(head_patch=hp, patch=dict(site=1, vectors=torch.zeros(5, c.hidden))),
                         "knockout": dict(head_patch=hp, knockout=([[0] * n for n in env.lens], [[]] * 4 + [[1]]))}.items():
            with pytest.raises(ValueError, match=word):
                rt.generate(env.prompts, env.sp, max_new_tokens=2, **kw)
        assert rt.ws.nbytes() == before and not calls
    finally:
        del rt.llama.prefill


# ------------------------------------------------------------------------------------------------------------------
# head_contrib
# ------------------------------------------------------------------------------------------------------------------
def test_head_contrib_against_float64(env):
    c = env.cfg.llama
    D, worst = c.head_dim, 0.0
    for layer in range(L):
        pairs = ALL(c, layer)[::-1]                                              # every head of the layer, in descending order
        got = env.rt.head_contrib(env.cap.head_out, pairs)
        assert got.shape == (5, c.n_heads, c.hidden) and got.dtype == torch.float32
        wo = env.rt.llama.w.layers[layer].wo
        total_ref = torch.zeros(5, c.hidden, dtype=torch.float64, device=DEV)
        total_bound = torch.zeros_like(total_ref)
        for i, (_, h) in enumerate(pairs):
            dot, mag = fb.dot64(env.cap.head_out[:, layer, h], wo[:, h * D:(h + 1) * D])
            ref, bound = fb.gemm_ref_bound(dot, mag, D)
            fb.assert_within(got[:, i], ref, bound, f"head_contrib layer {layer} head {h}")
            worst = max(worst, fb.worst_ratio(got[:, i], ref, bound))
            total_ref += ref
            total_bound += bound
        whole, _ = fb.dot64(env.cap.head_out[:, layer].flatten(1), wo)            # the o GEMM's product on the whole row
        assert bool(((total_ref - whole).abs() <= 2.0 ** -40 * (1 + whole.abs())).all())
        fb.assert_within(got.double().sum(1), whole, total_bound + 2.0 ** -40 * (1 + whole.abs()), f"head_contrib layer {layer}: the sum over heads")
    print(f"head_contrib kv={c.n_kv_heads} qk_norm={c.qk_norm}: largest err / bound {worst:.3f} (gemm_ref_bound at K = {D})")
    sub = env.rt.head_contrib(env.cap.head_out.cpu(), [(1, 2), (0, 0)])           # a CPU tensor, pairs in any order
    assert torch.equal(sub[:, 0], env.rt.head_contrib(env.cap.head_out, ALL(c, 1))[:, 2])


# ------------------------------------------------------------------------------------------------------------------
# against transformers
# ------------------------------------------------------------------------------------------------------------------
HF_PATCHES = {
    "zero-two-heads-prompt": dict(heads=[(1, 2), (0, 1)], mode="replace", steps="prompt", scale=0.0),
    "add-half-v-all": dict(heads=[(1, 2), (0, 1)], mode="add", alpha=0.5, steps="all", scale=1.0),
}
MIN_DECISIONS = 8


@pytest.mark.parametrize("name", list(HF_PATCHES))
def test_patched_run_against_transformers(env, name):
    p = dict(HF_PATCHES[name])
    scale = p.pop("scale")
    hp = dict(p, vectors=env.vectors(p["heads"]) * scale)
    res = env.gen(hp, want_heads=True)
    got, heads = res.step_logits.double().cpu(), res.head_out.double().cpu()
    hf = env.hf()
    want32, ho32 = ph.heads_run(env, hf, torch.float32, res.tokens, hp)
    want16, ho16 = ph.heads_run(env, hf, torch.bfloat16, res.tokens, hp)
    free32, _ = ph.heads_run(env, hf, torch.float32, res.tokens)
    c = env.cfg.llama
    tag = f"{name} kv={c.n_kv_heads} qk_norm={c.qk_norm}"
    for layer in range(L):
        own, mine = _rel(ho16[:, layer], ho32[:, layer]), _rel(heads[:, layer], ho32[:, layer])
        print(f"{tag} layer {layer} head_out: rel-L2 vs HF fp32 {mine:.3e}; HF bf16 vs HF fp32 {own:.3e}; ratio {mine / own:.3f} (allowed {PARITY_RATIO})")
        assert mine <= PARITY_RATIO * own, f"layer {layer}"
    ph.parity_check(got, want32, want16, free32, res.tokens, tag, effect_floor=0, min_decisive=MIN_DECISIONS)


# ------------------------------------------------------------------------------------------------------------------
# the plugin
# ------------------------------------------------------------------------------------------------------------------
def test_plugin():
    model, few, zero = ph.tiny_plugin_batches(2, 0)
    c = model.cfg.llama
    ho = model.head_outputs(dict(few))
    assert set(ho) == {"head_out", "first_logits", "tokens", "texts"} and ho["head_out"].shape == (2, c.n_layers, c.n_heads, c.head_dim)
    plain_few = model.generate_ids(dict(few), want_first_logits=True)
    assert torch.equal(ho["first_logits"], plain_few.first_logits) and torch.equal(ho["tokens"], plain_few.tokens)
    pairs = [(c.n_layers - 1, 1), (0, 0)]
    vec = torch.stack([ho["head_out"][:, l, h].float() for l, h in pairs], dim=1)
    with ph.spy_generate(model) as seen:
        out = model.generate_head_patched(dict(zero), pairs, vec)
    assert set(out) == {"texts", "tokens", "first_logits"} and len(out["texts"]) == 2 and out["first_logits"].shape == (2, c.vocab)
    hp = seen["kw"]["head_patch"]
    assert hp["heads"] == pairs and hp["mode"] == "replace" and hp["steps"] == "prompt" and hp["rows"] is None
    direct = model.runtime.generate(seen["segs"], seen["speech"], **seen["kw"])                 # the runtime-level call
    assert torch.equal(direct.first_logits, out["first_logits"]) and torch.equal(direct.tokens, out["tokens"])
    plain_zero = model.generate_ids(dict(zero), want_first_logits=True)
    assert not torch.equal(out["first_logits"], plain_zero.first_logits)
    abl = model.generate_head_patched(dict(zero), pairs, torch.zeros(2, c.head_dim), steps="all", rows=[1])     # a zero ablation of row 1
    assert torch.equal(abl["first_logits"][0], plain_zero.first_logits[0]) and not torch.equal(abl["first_logits"][1], plain_zero.first_logits[1])
    with pytest.raises(ValueError, match="shape"):
        model.generate_head_patched(dict(zero), pairs, vec[:, :1])
    with pytest.raises(ValueError, match="outside"):
        model.generate_head_patched(dict(zero), [(c.n_layers, 0)], vec[:, :1])
    # the function-vector recipe of the README: head outputs on few-shot prompts -> the mean of the heads' contributions to the
    # stream over prompts and pairs -> added to the stream of zero-shot prompts behind the last of those layers
    contrib = model.runtime.head_contrib(ho["head_out"], pairs)
    assert contrib.shape == (2, 2, c.hidden)
    fv = contrib.mean(dim=(0, 1))
    steered = model.generate_patched(dict(zero), fv, c.n_layers, mode="add", alpha=4.0)
    assert steered["first_logits"].shape == (2, c.vocab) and not torch.equal(steered["first_logits"], plain_zero.first_logits)
    assert torch.equal(model.generate_ids(dict(zero), want_first_logits=True).first_logits, plain_zero.first_logits)

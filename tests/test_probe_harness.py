"""CPU: tests/probe_harness.py, the harness of the decoder probes' runtime tests.

1. The inputs are pinned.  ``WEIGHT_SEED`` was picked for its greedy margins and README.md's figures were measured on exactly these
   weights and prompts, so SHA-256 digests of every harness variant the GPU modules build — the state dict (keys sorted, raw bytes),
   ``speech``, ``prompts``, ``lens`` and ``other`` — are compared with tests/golden/probe_harness_digests.json, recorded from the
   classes the modules held before they shared this harness.  The integer digests hold anywhere; the float ones (``randn`` and the
   bf16 rounding) are compared where torch is the version the file names.
2. ``parity_check`` passes on a run that is the bf16 reference itself and fails on each of its four conditions alone.
3. ``hf()`` loads strictly in both forms, and the teacher-forced run fires its hooks once per layer of the window.
"""
import hashlib
import json
import os

import pytest
import torch

import probe_harness as ph
from decoder_support import GOLDEN

PINS = json.load(open(os.path.join(GOLDEN, "probe_harness_digests.json")))
# the variants of the six GPU modules: constructor arguments behind (kv, qk_norm), and the forms each module runs
VARIANTS = {
    "knockout": (dict(n_layers=2), ("mha", "gqa", "gqa-qknorm")),
    "cuts": (dict(n_layers=3), ("mha", "gqa-qknorm")),
    "resid": (dict(n_layers=3, other=True), ("mha", "gqa-qknorm")),
    "head": (dict(n_layers=3, other=True), ("mha", "gqa-qknorm")),
    "segmass": (dict(n_layers=2, redraw=False, speech_scale=0.05), ("mha", "gqa", "gqa-qknorm", "mha-qknorm")),
    "segflow": (dict(n_layers=2, redraw=False, row_seed=29), ("mha", "gqa-qknorm")),
}
FORMS = {"mha": (None, False), "gqa": (2, False), "gqa-qknorm": (2, True), "mha-qknorm": (None, True)}
FLOAT_KEYS = ("sd", "speech")


def _sha(*chunks):
    h = hashlib.sha256()
    for c in chunks:
        h.update(c if isinstance(c, bytes) else json.dumps(c).encode())
    return h.hexdigest()


def _raw(t):
    return [str(t.dtype), list(t.shape)], t.contiguous().view(torch.uint8).numpy().tobytes()


def digests(env):
    """{"sd", "speech", "prompts", "lens", "other"}: SHA-256 of what a harness (of today or of the earlier classes) drew."""
    out = {"sd": _sha(*[x for k in sorted(env.sd) for x in (k, *_raw(env.sd[k]))]),
           "speech": None if getattr(env, "speech", None) is None else _sha(*_raw(env.speech)),
           "prompts": _sha(env.prompts),
           "lens": _sha(list(env.lens)),
           "other": _sha(env.other) if hasattr(env, "other") else None}
    return out


@pytest.mark.parametrize("variant,form", [(v, f) for v, (_, forms) in VARIANTS.items() for f in forms])
def test_the_harness_draws_what_the_modules_always_drew(variant, form):
    got = digests(ph.Decoder(*FORMS[form], **VARIANTS[variant][0]))
    want = PINS["digests"][f"{variant}/{form}"]
    assert set(got) == set(want)
    same_torch = torch.__version__ == PINS["torch"]
    for key in got:
        if key in FLOAT_KEYS and not same_torch:
            continue
        assert got[key] == want[key], (variant, form, key)
    assert (got["other"] is not None) == VARIANTS[variant][0].get("other", False)


# ------------------------------------------------------------------------------------------------------------------
# parity_check on synthetic tensors
# ------------------------------------------------------------------------------------------------------------------
def _synthetic():
    """want32 f64 [4, 5, 64] with a top-1 / top-2 margin of 1 at 12 of the 20 decisions and of 1e-6 at the others; want16 = want32
    + noise of at most 1e-3 per logit; free32 far from both."""
    g = torch.Generator().manual_seed(1)
    want32 = torch.rand(ph.NEW, 5, 64, generator=g, dtype=torch.float64)
    top = torch.randint(0, 64, (ph.NEW, 5), generator=g)
    wide = (torch.arange(20).reshape(ph.NEW, 5) % 5) < 3
    want32.scatter_(2, top[..., None], 2.0)
    want32.scatter_(2, ((top + 1) % 64)[..., None], torch.where(wide, 1.0, 2.0 - 1e-6)[..., None].double())
    noise = (torch.rand(want32.shape, generator=g, dtype=torch.float64) - 0.5) * 2e-3
    return want32, want32 + noise, want32 + 0.1, top.t().contiguous(), wide.t()


def _check(got, want32, want16, free32, tokens, effect_floor=4, min_decisive=12):
    ph.parity_check(got, want32, want16, free32, tokens, "synthetic", effect_floor=effect_floor, min_decisive=min_decisive)


def test_parity_check_passes_on_the_bf16_reference_itself():
    want32, want16, free32, tokens, wide = _synthetic()
    _check(want16, want32, want16, free32, tokens)
    _check(want32 + 1.2 * (want16 - want32), want32, want16, free32, tokens)            # ratio 1.2
    other = tokens.clone()
    other[~wide] = 0                                                                     # tokens at the undecisive margins are free
    _check(want16, want32, want16, free32, other)
    _check(want16, want32, want16, want32 + 1e-9, tokens, effect_floor=0)               # floor 0: any effect at all


def test_parity_check_fails_on_each_condition_alone():
    want32, want16, free32, tokens, wide = _synthetic()
    with pytest.raises(AssertionError, match=r"synthetic step 0(\n|$)"):                       # the ratio above 1.25, in one step
        got = want16.clone()
        got[0] = want32[0] + 1.3 * (want16[0] - want32[0])
        _check(got, want32, want16, free32, tokens)
    own = ph.rel(want16[2], want32[2])
    at_floor = free32.clone()
    at_floor[2] = want32[2] + (free32[2] - want32[2]) * (3.99 * own / ph.rel(free32[2], want32[2]))
    with pytest.raises(AssertionError, match="step 2: the intervention does not reach"):
        _check(want16, want32, want16, at_floor, tokens)
    with pytest.raises(AssertionError, match="does not reach"):                          # floor 0 means strictly positive
        _check(want16, want32, want16, want32, tokens, effect_floor=0)
    with pytest.raises(AssertionError, match="too few decisive"):
        _check(want16, want32, want16, free32, tokens, min_decisive=13)
    wrong = tokens.clone()
    b, t = [int(i) for i in wide.nonzero()[5]]
    wrong[b, t] = (wrong[b, t] + 1) % 64
    with pytest.raises(AssertionError, match="a decisive token differs"):
        _check(want16, want32, want16, free32, wrong)


# ------------------------------------------------------------------------------------------------------------------
# the transformers twin and the teacher-forced run
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["mha", "gqa-qknorm"])
def env(request):
    return ph.Decoder(*FORMS[request.param], n_layers=3, other=True)


def test_hf_loads_strictly_in_both_forms(env):
    m = env.hf()                                                                         # load_state_dict(strict=True) inside
    assert type(m).__name__ == ("Qwen3ForCausalLM" if env.cfg.llama.qk_norm else "LlamaForCausalLM")
    assert set(m.state_dict()) == {k[len("llama_model."):] for k in env.sd}
    for k, v in m.state_dict().items():
        assert torch.equal(v, env.sd["llama_model." + k]), k


def test_the_teacher_forced_run_fires_its_hooks_once_per_layer_of_the_window(env):
    c, m = env.cfg.llama, env.hf()
    tokens = ((3 + torch.arange(5 * ph.NEW)) % (c.vocab - 4)).reshape(5, ph.NEW)
    plain, fired = ph.masked_run(env, m, torch.float32, tokens, lambda b, n, dead: None, (1, 3))
    assert fired == [2] * 5 and plain.shape == (ph.NEW, 5, c.vocab) and plain.dtype == torch.float64
    calls = []

    def fill(b, n, dead):
        assert dead.shape == (n + ph.NEW - 1,) * 2 and n == env.lens[b]
        calls.append(b)
        dead[n - 1:, :2] = True
    cut, fired = ph.masked_run(env, m, torch.float32, tokens, fill, (0, 1))
    assert fired == [1] * 5 and calls == list(range(5)) and not torch.equal(cut, plain)
    assert not any(mod._forward_pre_hooks for mod in m.modules())                        # every handle was removed
    # the causal mask handed in is transformers' own: the residual and head hooks, which leave the mask alone, give the same logits
    lg, hidden, lens = ph.resid_run(env, m, torch.float32, tokens)
    assert torch.equal(lg, plain) and torch.allclose(lens[:, c.n_layers], plain[0], rtol=1e-5, atol=1e-5)
    lg, heads = ph.heads_run(env, m, torch.float32, tokens)
    assert torch.equal(lg, plain) and heads.shape == (5, c.n_layers, c.n_heads, c.head_dim)
    assert not any(mod._forward_pre_hooks for mod in m.modules())

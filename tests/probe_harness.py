"""What the runtime tests of the decoder probes share (tests/test_gpu_attn_knockout.py, test_gpu_cuts_runtime.py,
test_gpu_resid_patch_runtime.py, test_gpu_head_patch_runtime.py, test_gpu_attn_segmass.py, test_gpu_segflow_runtime.py): not a test
module.  Everything here runs on the CPU; only ``Decoder.runtime(device)`` builds the GPU side.

1. ``Decoder``: the small decoder (hidden 512, 4 heads of 128, no LoRA, so a transformers model holds the same tensors), its five
   ragged prompts and its transformers twin.  The tolerances in README.md were measured on exactly these draws, so their order is
   fixed — the weights in ``salmonn_state`` item order; then from ``Generator(17)`` the speech rows, each prompt's ids in order, and
   the second batch ``other`` — and tests/test_probe_harness.py pins digests of every variant in use.
2. ``teacher_forced``: transformers on prompt + the GPU's first NEW - 1 tokens under forward pre-hooks, and the three sets of hooks:
   a 4-D additive mask for a layer window (``masked_run``), the residual sites (``resid_run``), the ``o_proj`` inputs (``heads_run``).
3. ``parity_check``: the project's criterion for an intervention's logits and greedy tokens against transformers.
4. Small helpers of the bit-for-bit and plugin tests.
"""
from contextlib import contextmanager
from dataclasses import replace

import torch

from decoder_support import row_prompts, salmonn_batch

PARITY_RATIO = 1.25
PROMPT_LENS = [33, 90, 61, 12, 130]
SPEECH_ROW, SPEECH_AT, SPEECH_N = 1, 20, 17          # prompt 1 carries 17 speech rows after its 20th token
OTHER_LENS = (40, 17, 77, 25, 101)
NEW = 4
# of 40 seeds, the one with the widest smallest fp32 greedy margin of transformers on the CPU at 2 layers; the two conditions on the
# reference alone were re-checked at 3
WEIGHT_SEED = 10_005


# ------------------------------------------------------------------------------------------------------------------
# 1. the decoder
# ------------------------------------------------------------------------------------------------------------------
class Decoder:
    """``n_layers`` layers, ``kv`` K/V heads (None: multi-head), Qwen3's q/k norms with ``qk_norm``.  ``redraw``: every matrix drawn
    again from ``WEIGHT_SEED``, layer projections small (std 0.03) next to the embeddings and the LM head (0.3), rounded through
    bf16; else the ``synth.salmonn_state`` weights as they are.  Prompts: ``row_prompts(vocab, PROMPT_LENS, row_seed)`` and no
    speech, or (``row_seed`` None) ids and ``speech`` rows of std ``speech_scale`` from ``Generator(17)``, prompt 1 with a speech
    segment, and with ``other`` a second batch of five.  ``lens``: the prompts' positions."""

    def __init__(self, kv, qk_norm, n_layers, *, redraw=True, speech_scale=0.3, row_seed=None, other=False):
        from icl_speech_text_llm_amd.runtime import synth
        from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
        from icl_speech_text_llm_amd.runtime.salmonn import speech_segment
        tiny = SalmonnCfg.tiny(use_beats=False, lora=False)
        self.cfg = replace(tiny, llama=replace(tiny.llama, hidden=512, n_layers=n_layers, n_heads=4, n_kv_heads=kv, ffn=1024, qk_norm=qk_norm))
        c = self.cfg.llama
        self.sd = synth.salmonn_state(self.cfg, seed=0, jitter=True, parts=("llama",))
        if redraw:
            g = torch.Generator().manual_seed(WEIGHT_SEED)
            for k, v in self.sd.items():
                if v.dim() > 1:
                    self.sd[k] = (torch.randn(v.shape, generator=g) * (0.03 if "_proj" in k else 0.3)).to(torch.bfloat16).float()
        if row_seed is not None:
            self.speech, self.prompts, self.lens = None, row_prompts(c.vocab, PROMPT_LENS, row_seed), list(PROMPT_LENS)
            return
        g = torch.Generator().manual_seed(17)
        draw = lambda n: torch.randint(3, c.vocab - 1, (n,), generator=g).tolist()
        self.speech = torch.randn(SPEECH_N + 3, c.hidden, generator=g) * speech_scale
        self.prompts = [[draw(n)] for n in PROMPT_LENS]
        ids = self.prompts[SPEECH_ROW][0]
        self.prompts[SPEECH_ROW] = [ids[:SPEECH_AT], speech_segment(2, SPEECH_N), ids[SPEECH_AT:]]
        self.lens = [n + (SPEECH_N if b == SPEECH_ROW else 0) for b, n in enumerate(PROMPT_LENS)]
        if other:
            self.other = [[draw(n)] for n in OTHER_LENS]

    def runtime(self, device, **kw):
        from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
        return SalmonnRuntime(self.cfg, dict(self.sd), device=device, parts=("llama",), **kw)

    def hf(self):
        """The same tensors as a transformers model on the CPU (Qwen3 with ``qk_norm``, else Llama), eager attention."""
        import transformers as tf
        c = self.cfg.llama
        assert c.rope_theta == 10000.0                     # the default of both configurations
        kw = dict(hidden_size=c.hidden, num_hidden_layers=c.n_layers, num_attention_heads=c.n_heads, num_key_value_heads=c.kv_heads,
                  intermediate_size=c.ffn, vocab_size=c.vocab, rms_norm_eps=c.rms_eps, max_position_embeddings=c.max_pos,
                  tie_word_embeddings=False, attention_bias=False, head_dim=c.head_dim, attn_implementation="eager")
        m = (tf.Qwen3ForCausalLM(tf.Qwen3Config(**kw)) if c.qk_norm else tf.LlamaForCausalLM(tf.LlamaConfig(**kw))).eval()
        m.load_state_dict({k[len("llama_model."):]: v for k, v in self.sd.items()}, strict=True)
        return m


def four_runs(n, at=None):
    """Segment ids of ``n`` positions in four equal runs 0 .. 3, with the ids of ``at`` = {position: id} put over them."""
    sg = [j * 4 // n for j in range(n)]
    for j, g in (at or {}).items():
        sg[j] = g
    return sg


def speech_row_runs():
    """Segment ids of the prompt with the speech segment: the text before it, the speech rows, the text after them."""
    return [0] * SPEECH_AT + [1] * SPEECH_N + [2] * (PROMPT_LENS[SPEECH_ROW] - SPEECH_AT)


# ------------------------------------------------------------------------------------------------------------------
# 2. transformers, teacher-forced along the GPU's tokens
# ------------------------------------------------------------------------------------------------------------------
def teacher_forced(env, m, dtype, tokens, install):
    """transformers model ``m`` in ``dtype`` on every prompt + the first NEW - 1 tokens of ``tokens`` [B, NEW], eager attention.
    ``install(m, b, n)`` registers the hooks of prompt ``b`` (``n`` positions) and returns (their handles, what they collect); the
    handles are removed whatever happens.  -> (logits at positions n - 1 .. n + NEW - 2, f64 [NEW, B, V]; the collections)."""
    m, c = m.to(dtype), env.cfg.llama
    emb = m.get_input_embeddings().weight.detach().float()
    logits = torch.zeros(NEW, len(env.prompts), c.vocab, dtype=torch.float64)
    collected = []
    for b, segs in enumerate(env.prompts):
        x = torch.cat([env.speech[s[1]:s[1] + s[2]] if isinstance(s, tuple) else emb[torch.tensor(s)] for s in segs]
                      + [emb[tokens[b, :NEW - 1]]])
        n = env.lens[b]
        hooks, got = install(m, b, n)
        try:
            with torch.no_grad():
                lg = m(inputs_embeds=x[None].to(dtype)).logits[0]
        finally:
            for h in hooks:
                h.remove()
        logits[:, b] = lg[n - 1:].double()
        collected.append(got)
    return logits, collected


def masked_run(env, m, dtype, tokens, fill_dead, window):
    """Teacher-forced under a 4-D additive mask given to the decoder layers ``range(*window)`` by a forward pre-hook (the others
    keep the causal mask).  ``fill_dead(b, n, dead)`` adds prompt ``b``'s blocked (row, column) pairs to the causal bool
    [T, T] ``dead``, T = n + NEW - 1.  -> (step logits f64 [NEW, B, V], the number of hooks that fired per prompt)."""
    def install(m, b, n):
        T = n + NEW - 1
        dead = torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
        fill_dead(b, n, dead)
        mask = torch.zeros(T, T, dtype=dtype).masked_fill(dead, float("-inf"))[None, None]
        seen = []

        def hook(mod, args, kwargs):
            assert "attention_mask" in kwargs, "the decoder layers do not take the mask as a keyword"
            seen.append(1)
            return args, dict(kwargs, attention_mask=mask)
        return [m.model.layers[i].register_forward_pre_hook(hook, with_kwargs=True) for i in range(*window)], seen
    logits, seen = teacher_forced(env, m, dtype, tokens, install)
    return logits, [len(s) for s in seen]


def _rewrite(x, rows, v, p):
    """Rows ``rows`` of ``x`` replaced by ``v`` or given alpha times ``v``, as patch ``p`` (mode, alpha) says; in place."""
    x[rows] = v if p.get("mode", "replace") == "replace" else x[rows] + p.get("alpha", 1.0) * v


def _patched_rows(p, n):
    """The last prompt row, with ``steps="all"`` every later row too."""
    return slice(n - 1, None) if p.get("steps", "prompt") == "all" else slice(n - 1, n)


def resid_run(env, m, dtype, tokens, patch=None):
    """Teacher-forced with forward pre-hooks on the decoder layers and on ``model.norm`` that read the residual stream at every
    site and, with ``patch`` = dict(site, vectors f32 [B, hidden] | [1, hidden], mode, alpha, steps, rows | None), rewrite it at
    one: the last prompt row (``steps="all"``: and every later row) of a listed prompt is replaced by, or gets alpha times, its
    vector.  -> (step logits f64 [NEW, B, V], hidden f64 [B, n_layers + 1, hidden]: the last prompt row at every site, pre-patch,
    lens logits f64 [B, n_layers + 1, V]: model.norm + lm_head on those rows)."""
    c = env.cfg.llama

    def install(m, b, n):
        seen, kept = [], {}

        def hook(mod, args, kwargs, site):
            hs = args[0] if args else kwargs["hidden_states"]
            seen.append(site)
            kept[site] = hs[:, n - 1:n].clone()
            if patch is None or patch["site"] != site or (patch.get("rows") is not None and b not in patch["rows"]):
                return None
            v = patch["vectors"]
            hs = hs.clone()
            _rewrite(hs[0], _patched_rows(patch, n), (v[0] if v.shape[0] == 1 else v[b]).to(hs.dtype), patch)
            return ((hs,) + tuple(args[1:]), kwargs) if args else (args, dict(kwargs, hidden_states=hs))
        mods = list(m.model.layers) + [m.model.norm]
        return [mod.register_forward_pre_hook(lambda mo, a, k, s=s: hook(mo, a, k, s), with_kwargs=True) for s, mod in enumerate(mods)], (seen, kept)
    logits, got = teacher_forced(env, m, dtype, tokens, install)
    hidden = torch.zeros(len(got), c.n_layers + 1, c.hidden, dtype=torch.float64)
    lens_logits = torch.zeros(len(got), c.n_layers + 1, c.vocab, dtype=torch.float64)
    with torch.no_grad():                                   # the hooks are gone: model.norm can be used for the lens
        for b, (seen, kept) in enumerate(got):
            assert seen == list(range(c.n_layers + 1)), seen
            for site, row in kept.items():
                hidden[b, site] = row[0, 0].double()
                lens_logits[b, site] = m.lm_head(m.model.norm(row))[0, 0].double()
    return logits, hidden, lens_logits


def heads_run(env, m, dtype, tokens, hp=None):
    """Teacher-forced with a forward pre-hook on every layer's ``self_attn.o_proj`` that reads its input's last prompt row and,
    with ``hp`` = dict(heads, vectors f32 [B, n_pairs, D] | [1, n_pairs, D], mode, alpha, steps, rows | None), rewrites the selected
    heads of that row (``steps="all"``: and of every later row).  -> (step logits f64 [NEW, B, V], head_out f64 [B, L, H, D],
    pre-patch)."""
    c = env.cfg.llama
    H, D = c.n_heads, c.head_dim
    head_out = torch.zeros(len(env.prompts), c.n_layers, H, D, dtype=torch.float64)

    def install(m, b, n):
        seen = []

        def hook(mod, args, layer):
            a = args[0]
            seen.append(layer)
            head_out[b, layer] = a[0, n - 1].double().view(H, D)
            mine = [(s, h) for s, (l, h) in enumerate(hp["heads"]) if l == layer] if hp is not None else []
            if not mine or (hp.get("rows") is not None and b not in hp["rows"]):
                return None
            a = a.clone()
            for s, h in mine:
                v = hp["vectors"]
                _rewrite(a[0, :, h * D:(h + 1) * D], _patched_rows(hp, n), (v[0, s] if v.shape[0] == 1 else v[b, s]).to(a.dtype), hp)
            return (a,) + tuple(args[1:])
        return [lay.self_attn.o_proj.register_forward_pre_hook(lambda mo, a, i=i: hook(mo, a, i)) for i, lay in enumerate(m.model.layers)], seen
    logits, seen = teacher_forced(env, m, dtype, tokens, install)
    assert seen == [list(range(c.n_layers))] * len(env.prompts), seen
    return logits, head_out


# ------------------------------------------------------------------------------------------------------------------
# 3. the criterion
# ------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    return float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float((a - b).norm())


def parity_check(got, want32, want16, free32, tokens, tag, *, effect_floor, min_decisive, moves="the patch moves"):
    """The GPU's step logits ``got`` and greedy ``tokens`` [B, NEW] under an intervention, against transformers under the same
    intervention in fp32 (``want32``) and in bf16 (``want16``) and without it in fp32 (``free32``), all f64 [NEW, B, V].  Per step:
    rel-L2(got, want32) <= PARITY_RATIO x own, own = rel-L2(want16, want32), and the intervention moves transformers' own logits
    by more than ``effect_floor`` x own (0: at all) — else the reference would prove nothing.  Tokens: equal to want32's arg-max
    wherever its margin is decisive.  With random logits some top-1 / top-2 gaps are always next to nothing, so "decisive" is
    decided on the reference alone: a gap above 2 x PARITY_RATIO x the largest |want16 - want32| logit error (both sides of the gap
    may move by the allowed error); at least ``min_decisive`` decisions must be that decisive.  Prints every figure."""
    for t in range(got.shape[0]):
        own, mine, effect = rel(want16[t], want32[t]), rel(got[t], want32[t]), rel(free32[t], want32[t])
        print(f"{tag} step {t}: rel-L2 vs HF fp32 {mine:.3e}; HF bf16 vs HF fp32 {own:.3e}; ratio {mine / own:.3f} (allowed "
              f"{PARITY_RATIO}); {moves} HF's logits by {effect:.3e} ({effect / own:.1f} x)")
        assert effect > effect_floor * own, f"{tag} step {t}: the intervention does not reach transformers: the reference would prove nothing"
        assert mine <= PARITY_RATIO * own, f"{tag} step {t}"
    top2 = want32.topk(2, dim=-1).values
    margin = (top2[..., 0] - top2[..., 1]).t()                                   # [B, NEW]
    noise = float((want16 - want32).abs().max())
    decisive = margin > 2 * PARITY_RATIO * noise
    print(f"{tag}: top-1 / top-2 margins of HF fp32: {int(decisive.sum())} of {decisive.numel()} above {2 * PARITY_RATIO * noise:.3f} "
          f"(smallest {float(margin.min()):.3f}); largest |logit difference| to HF fp32 {float((got - want32).abs().max()):.3e}")
    assert int(decisive.sum()) >= min_decisive, f"{tag}: too few decisive margins"
    assert torch.equal(tokens[decisive], want32.argmax(-1).t()[decisive]), f"{tag}: a decisive token differs"


# ------------------------------------------------------------------------------------------------------------------
# 4. small helpers
# ------------------------------------------------------------------------------------------------------------------
def same_result(a, b):
    return torch.equal(a.tokens, b.tokens) and torch.equal(a.first_logits, b.first_logits) and torch.equal(a.step_logits, b.step_logits)


@contextmanager
def prefill_chunks(rt, n):
    """Prefill in chunks of ``n`` sequences inside the block."""
    rt.prefill_chunk = n
    try:
        yield
    finally:
        del rt.prefill_chunk


def tiny_plugin_batches(*num_examples):
    """The tiny SALMONN plugin on the GPU and, per entry, its first speech batch of two with that many few-shot examples."""
    from icl_speech_text_llm_amd.models.model_factory import ModelFactory
    model = ModelFactory.create_model("salmonn", device="cuda", arch="tiny", low_resource=True, llama_path="none", lora_alpha=32).eval()
    on_gpu = lambda b: {k: (v.to("cuda") if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
    return (model,) + tuple(on_gpu(salmonn_batch(model, "speech", n=2, bs=2, num_examples=k)) for k in num_examples)


@contextmanager
def spy_generate(model):
    """Inside the block ``model.runtime.generate`` records its last call: yields the dict of ``segs``, ``speech``, ``kw``, ``result``."""
    seen = {}
    real = model.runtime.generate

    def generate(segs, speech, **kw):
        seen.update(segs=segs, speech=speech, kw=kw)
        seen["result"] = real(segs, speech, **kw)
        return seen["result"]
    model.runtime.generate = generate
    try:
        yield seen
    finally:
        del model.runtime.generate

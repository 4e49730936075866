"""`-m gpu`: ``generate(cuts=...)`` — attention cuts between prompt segments, edges whose QUERY is an interior prompt row — on the
harness of tests/probe_harness.py, which tests/test_gpu_attn_knockout.py uses at two layers, at THREE (hidden 512, 4 heads of 128:
multi-head with the trimmed last layer, and grouped 4 / 2 with QK-norm), five ragged prompts of 33 / 90 / 61 / 12 / 130 positions in
four equal segment runs, one with a speech segment, four new tokens.

Bit for bit: cuts on interior rows in the last layer alone are the plain run (no other row of that layer can influence anything);
prefill chunks of two are one chunk; a replayed decode graph is the eager run; in a mixed batch the prompts without pairs are the
plain run at every step; ``overlong="drop"`` gives the survivors what they get alone; ``want_hidden`` / ``want_heads`` change nothing.

Against transformers in fp32 on the CPU, eager attention under the 4-D additive mask of the cuts (row i, column j at -inf when j > i
or seg[j] is cut for seg[i]; generated keys 255, generated queries under ``generated``), given to the decoder layers of the window,
teacher-forced along the GPU's tokens — the knockout's three assertions per step: rel-L2(GPU, HF fp32) <= 1.25 x rel-L2(HF bf16, HF
fp32); the cut moves HF's logits by more than 4 x HF's bf16 error; the GPU's greedy tokens are HF fp32's wherever HF's margin exceeds
2 x 1.25 x its largest bf16 logit error, at least a third of the 20 decisions being that decisive.

Measured on MI355X: see README.md ("Attention cuts").
"""
import pytest
import torch

import probe_harness as ph
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)
from probe_harness import same_result as _same

pytestmark = pytest.mark.gpu

NEW = ph.NEW
N_LAYERS = 3
INTERIOR = dict(pairs=[(1, 0), (2, 1)], generated=255)        # no last row (segment 3) and no generated row is touched
DECIDING = dict(pairs=[(1, 0), (3, 1)], generated=3)          # the last rows and the generated rows do not read segment 1
CASES = {"interior-layers-0-2": (INTERIOR, (0, 2)), "interior-layer-0": (INTERIOR, (0, 1)), "interior-and-deciding-all-layers": (DECIDING, None)}


class _Env3(ph.Decoder):
    """The harness's decoder at 3 layers on the GPU; four equal segment runs per prompt (the speech rows of prompt 1 fall where
    they fall)."""

    def __init__(self, kv, qk_norm):
        super().__init__(kv, qk_norm, n_layers=N_LAYERS)
        self.rt = self.runtime(DEV)
        self.segments = [ph.four_runs(n) for n in self.lens]

    def cuts(self, case, layers=None, **kw):
        return dict(segments=self.segments, layers=layers, **{**case, **kw})

    def hf_cut_logits(self, m, dtype, tokens, pairs, generated, layers):
        """f64 [NEW, B, V]: transformers, teacher-forced, under the cuts' mask in the decoder layers of the window.  ``pairs``: one
        list for all prompts."""
        def fill_dead(b, n, dead):
            key_ids = torch.tensor(self.segments[b] + [255] * (NEW - 1))
            query_ids = torch.tensor(self.segments[b] + [generated] * (NEW - 1))
            for qs, ks in pairs:
                dead |= (query_ids == qs)[:, None] & (key_ids == ks)[None]
            assert not bool(dead.all(1).any())
        out, fired = ph.masked_run(self, m, dtype, tokens, fill_dead, layers)
        assert fired == [layers[1] - layers[0]] * len(self.prompts)
        return out


@pytest.fixture(scope="module", params=[(None, False), (2, True)], ids=["mha", "gqa-qknorm"])
def env(request):
    return _Env3(*request.param)


KW = dict(max_new_tokens=NEW, suppress_eos=True, want_first_logits=True, want_step_logits=True)


@pytest.fixture(scope="module")
def plain(env):
    return env.rt.generate(env.prompts, env.speech.to(DEV), **KW)


@pytest.mark.parametrize("name", list(CASES))
def test_runtime_against_transformers(env, plain, name):
    case, layers = CASES[name]
    rt, c = env.rt, env.cfg.llama
    res = rt.generate(env.prompts, env.speech.to(DEV), cuts=env.cuts(case, layers), **KW)
    assert res.tokens.shape == (len(env.prompts), NEW) and torch.equal(res.first_logits, res.step_logits[0])
    got = res.step_logits.double().cpu()
    window = (0, c.n_layers) if layers is None else layers
    hf = env.hf()
    want32 = env.hf_cut_logits(hf, torch.float32, res.tokens, case["pairs"], case["generated"], window)
    want16 = env.hf_cut_logits(hf, torch.bfloat16, res.tokens, case["pairs"], case["generated"], window)
    free32 = env.hf_cut_logits(hf, torch.float32, res.tokens, [], 255, window)
    ph.parity_check(got, want32, want16, free32, res.tokens, f"cuts {name} kv={c.n_kv_heads} qk_norm={c.qk_norm}",
                    effect_floor=4, min_decisive=res.tokens.numel() // 3 + 1, moves="the cuts move")
    assert not torch.equal(res.step_logits, plain.step_logits)


def test_interior_cuts_in_the_last_layer_alone_are_the_plain_run(env, plain):
    """Only the sequences' last rows of the last layer reach anything: interior cuts there move nothing, and launch nothing."""
    res = env.rt.generate(env.prompts, env.speech.to(DEV), cuts=env.cuts(INTERIOR, (N_LAYERS - 1, N_LAYERS)), **KW)
    assert _same(res, plain)
    # ... while the same window with the deciding rows in it is another run, and equals all layers' where only it differs
    last = env.rt.generate(env.prompts, env.speech.to(DEV), cuts=env.cuts(DECIDING, (N_LAYERS - 1, N_LAYERS)), **KW)
    assert not torch.equal(last.step_logits, plain.step_logits)


def test_chunks_graph_replay_and_captures_change_nothing(env):
    rt, sp = env.rt, env.speech.to(DEV)
    for case, layers in ((INTERIOR, (0, 2)), (DECIDING, None)):
        first = rt.generate(env.prompts, sp, cuts=env.cuts(case, layers), **KW)
        with ph.prefill_chunks(rt, 2):
            assert _same(rt.generate(env.prompts, sp, cuts=env.cuts(case, layers), **KW), first), "prefill chunks of two"
        for what in ("captures the decode graph", "replays it"):        # the first call of the key ran eagerly
            assert _same(rt.generate(env.prompts, sp, cuts=env.cuts(case, layers), **KW), first), what
        both = rt.generate(env.prompts, sp, cuts=env.cuts(case, layers), want_hidden=True, want_heads=True, **KW)
        assert _same(both, first) and both.hidden is not None and both.head_out is not None
        assert bool(torch.isfinite(both.hidden).all()) and bool(torch.isfinite(both.head_out.float()).all())
        heads = rt.generate(env.prompts, sp, cuts=env.cuts(case, layers, heads=[1, 3]), **KW)
        assert not torch.equal(heads.step_logits, first.step_logits)


def test_mixed_batch_and_overlong_drop(env, plain):
    rt, c, sp = env.rt, env.cfg.llama, env.speech.to(DEV)
    pairs = [DECIDING["pairs"], [], INTERIOR["pairs"], [], []]
    gen = [3, 3, 255, 255, 1]
    mixed = rt.generate(env.prompts, sp, cuts=dict(segments=env.segments, pairs=pairs, generated=gen), **KW)
    for b, pr in enumerate(pairs):
        same = torch.equal(mixed.step_logits[:, b], plain.step_logits[:, b]) and torch.equal(mixed.tokens[b], plain.tokens[b])
        assert same == (not pr), b
    alone = rt.generate(env.prompts, sp, cuts=env.cuts(DECIDING), **KW)
    assert torch.equal(mixed.step_logits[:, 0], alone.step_logits[:, 0])
    long_row = [[5] * (c.max_pos - 1)]
    res = rt.generate(env.prompts + [long_row], sp, overlong="drop", cuts=dict(segments=env.segments + [[0] * (c.max_pos - 1)],
                                                                               pairs=pairs + [[]], generated=gen + [0]), **KW)
    assert res.dropped == (5,) and torch.equal(res.step_logits[:, :5], mixed.step_logits) and torch.equal(res.tokens[:5], mixed.tokens)


def test_other_tails(env):
    from icl_speech_text_llm_amd.runtime.constraints import LabelAutomaton
    rt, c, sp = env.rt, env.cfg.llama, env.speech.to(DEV)
    auto = LabelAutomaton([0, 2, 3, 4], [10, 12, 11, c.eos_id], [1, 2, 2, 2], {}, c.vocab, c.eos_id)
    res = rt.generate(env.prompts, sp, max_new_tokens=NEW, cuts=env.cuts(DECIDING), constraint=(auto, [0] * 5))
    for b in range(5):
        assert [t for t in res.tokens[b].tolist() if t not in (c.eos_id, c.pad_id)] in ([10, 11], [12]), (b, res.tokens[b].tolist())
    draws = [rt.generate(env.prompts, sp, max_new_tokens=NEW, suppress_eos=True, do_sample=True, top_k=5, temperature=0.7,
                         generator=torch.Generator().manual_seed(99), cuts=env.cuts(DECIDING)).tokens for _ in range(2)]
    assert torch.equal(draws[0], draws[1]) and draws[0].shape == (5, NEW)


def test_refusals_launch_nothing(env):
    rt, sp = env.rt, env.speech.to(DEV)
    calls = []
    real = rt.llama.prefill
    rt.llama.prefill = lambda *a, **kw: calls.append(1) or real(*a, **kw)
    try:
        before = rt.ws.nbytes()
        for bad, word in ((env.cuts(DECIDING, pairs=[(1, 32)]), "0..31"), (env.cuts(DECIDING, (0, 4)), "layer window"),
                          (env.cuts(DECIDING, pairs=[(0, 0)]), "prompt 0, position 0"), (dict(segments=env.segments[:-1], pairs=[]), "for 5 prompts")):
            with pytest.raises(ValueError, match=word):
                rt.generate(env.prompts, sp, max_new_tokens=2, cuts=bad)
        with pytest.raises(ValueError, match="num_beams"):
            rt.generate(env.prompts, sp, max_new_tokens=2, cuts=env.cuts(DECIDING), num_beams=2)
        assert rt.ws.nbytes() == before and not calls
    finally:
        del rt.llama.prefill


def test_plugin():
    model, b = ph.tiny_plugin_batches(2)
    with ph.spy_generate(model) as seen:
        out = model.generate_cut(dict(b), [(("example", 1), ("example", 0)), (("speech", 0), ("example", 1))], generated=("speech", 0))
    assert set(out) == {"texts", "tokens", "first_logits", "pieces"}
    c = model.cfg.llama
    assert len(out["texts"]) == 2 and out["tokens"].shape[0] == 2 and out["first_logits"].shape == (2, c.vocab)
    assert out["pieces"] == model.prompt_attention(dict(b))["pieces"]
    ct = seen["kw"]["cuts"]
    ids = lambda pc, *ps: [pc.index(p) for p in ps]
    assert ct["layers"] is None and ct["heads"] is None and ct["generated"] == [pc.index(("speech", 0)) for pc in out["pieces"]]
    assert ct["pairs"] == [[tuple(ids(pc, ("example", 1), ("example", 0))), tuple(ids(pc, ("speech", 0), ("example", 1)))] for pc in out["pieces"]]
    for sg, pc in zip(ct["segments"], out["pieces"]):
        assert sorted(set(sg)) == list(range(len(pc)))
    assert out["tokens"] is seen["result"].tokens and out["first_logits"] is seen["result"].first_logits      # the runtime's, as they are
    plain = model.generate_ids(dict(b), want_first_logits=True)
    assert not torch.equal(out["first_logits"], plain.first_logits)
    per_row = model.generate_cut(dict(b), [[(("example", 1), ("example", 0))], []], layers=(0, 1), heads=[0])
    assert torch.equal(per_row["first_logits"][1], plain.first_logits[1]) and not torch.equal(per_row["first_logits"][0], plain.first_logits[0])
    with pytest.raises(ValueError, match="row 0.*no piece"):
        model.generate_cut(dict(b), [(("example", 7), ("example", 1))])
    with pytest.raises(ValueError, match="2 rows"):
        model.generate_cut(dict(b), [[], [], []])
    assert torch.equal(model.generate_ids(dict(b), want_first_logits=True).first_logits, plain.first_logits)

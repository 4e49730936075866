"""End-to-end parity of the HIP kernel chains (runtime/engines.py, runtime/salmonn.py) against the CPU
oracle (oracle/models.py) on identical seeded weights and inputs, at miniature shapes (`-m gpu`).

Two comparisons per stage:
  * oracle with the bf16 rounding hook (same rounding points as the HIP path)  -> tight tolerance;
  * oracle in pure fp32 (the reference's CPU behaviour)                         -> bf16-level tolerance.
Tolerances are relative L2 errors over the whole tensor, stated next to each assert.
"""
import numpy as np
import pytest
import torch

from decoder_support import row_prompts
from gpu_support import DEV, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _rel(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def env():
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    cfg = SalmonnCfg.tiny(use_beats=True, lora=True)
    sd = synth.salmonn_state(cfg, seed=0, jitter=True)
    rt = SalmonnRuntime(cfg, dict(sd), device=DEV)
    return cfg, sd, rt


def _wavs(lens, L=None, seed=1234):
    L = L or max(lens)
    wav = torch.zeros(len(lens), L)
    for i, n in enumerate(lens):
        rng = np.random.default_rng(seed + i)
        wav[i, :n] = torch.from_numpy(np.clip(rng.normal(0, 0.1, n), -1, 1).astype(np.float32))
    return wav


def test_whisper_encoder(env):
    from oracle import audio_frontend as af, models as om
    cfg, sd, rt = env
    lens = [48000, 480000]
    wav = _wavs(lens)
    spec = torch.stack([torch.from_numpy(af.whisper_logmel(wav[i, :n].numpy())) for i, n in enumerate(lens)])
    xt = rt.logmel.from_spectrogram(rt.ws, spec.to(DEV))
    got = rt.whisper.forward(rt.ws, xt).view(2, 1500, -1)
    ref_b = om.whisper_encoder(sd, spec, cfg.whisper.n_heads, "speech_encoder.", rnd=om.bf16_round)
    ref_f = om.whisper_encoder(sd, spec, cfg.whisper.n_heads, "speech_encoder.")
    eb, ef = _rel(got, ref_b), _rel(got, ref_f)
    print(f"whisper: rel err vs bf16-rounding oracle {eb:.2e}, vs fp32 oracle {ef:.2e}")
    assert eb < 2.5e-3 and ef < 6e-3            # measured on MI355X: 1.2e-3 / 2.7e-3


def test_beats_encoder(env):
    from oracle import models as om
    cfg, sd, rt = env
    lens = [16000 * 3 + 123, 16000 * 5]
    L = max(lens)
    wav = _wavs(lens, L)
    # (a) batch-1 semantics: every audio at its own length
    got, cu, T = rt.beats.forward(rt.ws, wav.to(DEV), lens, lens)
    got = got.clone()
    for i, n in enumerate(lens):
        ref_b, pm = om.beats_encoder(sd, wav[i:i + 1, :n], [n], prefix="beats.", n_heads=cfg.beats.n_heads, rnd=om.bf16_round)
        ref_f, _ = om.beats_encoder(sd, wav[i:i + 1, :n], [n], prefix="beats.", n_heads=cfg.beats.n_heads)
        assert ref_b.shape[1] == T[i] and not pm.any()
        eb, ef = _rel(got[cu[i]:cu[i + 1]], ref_b[0]), _rel(got[cu[i]:cu[i + 1]], ref_f[0])
        print(f"beats[{i}] T={T[i]}: rel err vs bf16-rounding oracle {eb:.2e}, vs fp32 oracle {ef:.2e}")
        assert eb < 2e-4 and ef < 8e-3              # measured: 6.4e-5 / 3.7e-3
    # (b) padded-batch semantics (speech exemplars): both audios run at L with a key padding mask
    got, cu, T = rt.beats.forward(rt.ws, wav.to(DEV), [L, L], lens)
    ref_b, pm = om.beats_encoder(sd, wav, lens, prefix="beats.", n_heads=cfg.beats.n_heads, rnd=om.bf16_round)
    assert pm[0].any()
    for i in range(2):
        valid = ~pm[i]
        eb = _rel(got[cu[i]:cu[i + 1]][valid], ref_b[i][valid])
        print(f"beats padded[{i}]: valid rows {int(valid.sum())}/{T[i]} rel err {eb:.2e}")
        assert eb < 2e-4                             # measured: 6.5e-5


def test_encode_speech_full(env):
    from oracle import audio_frontend as af, models as om
    cfg, sd, rt = env
    lens = [16000 * 4, 16000 * 6 + 77]
    wav = _wavs(lens)
    got = rt.encode_speech(wav, lens).clone()
    assert got.shape == (2, 88, cfg.llama.hidden)
    for i, n in enumerate(lens):
        spec = torch.from_numpy(af.whisper_logmel(wav[i, :n].numpy()))[None]
        ref_b = om.salmonn_encode_speech(sd, spec, wav[i:i + 1, :n], [n], cfg.whisper.n_heads, rnd=om.bf16_round,
                                         beats_cfg=dict(n_heads=cfg.beats.n_heads), qformer_heads=cfg.qformer.n_heads)
        ref_f = om.salmonn_encode_speech(sd, spec, wav[i:i + 1, :n], [n], cfg.whisper.n_heads,
                                         beats_cfg=dict(n_heads=cfg.beats.n_heads), qformer_heads=cfg.qformer.n_heads)
        eb, ef = _rel(got[i], ref_b[0]), _rel(got[i], ref_f[0])
        print(f"encode_speech[{i}]: rel err vs bf16-rounding oracle {eb:.2e}, vs fp32 oracle {ef:.2e}")
        assert eb < 1.5e-3 and ef < 5e-3            # measured: 7.2e-4 / 2.2e-3
    # spectrogram supplied by the caller (the reference's batch dict) must give the same result as in-path K1
    spec_in = rt.log_mel(wav, lens).clone()
    got2 = rt.encode_speech(wav, lens, spectrogram=spec_in)
    assert _rel(got2, got) < 1e-6


def _llama_oracle(cfg, sd, rnd=None):
    from oracle import models as om
    lsd = {k[len("llama_model."):]: v for k, v in sd.items() if k.startswith("llama_model.")}
    return om.LlamaOracle(lsd, cfg.llama.n_heads, cfg.llama.rms_eps, cfg.llama.rope_theta, cfg.llama.lora_scale, rnd=rnd)


def _prompts(cfg, lens, n_speech=0, seed=99):
    from icl_speech_text_llm_amd.runtime.salmonn import speech_segment
    rows = row_prompts(cfg.llama.vocab, lens, seed)
    if not n_speech:
        return rows
    return [[ids[:len(ids) // 2], speech_segment(i * n_speech, n_speech), ids[len(ids) // 2:]] for i, (ids,) in enumerate(rows)]


def test_llama_forward_logits_and_loss(env):
    from oracle import models as om
    cfg, sd, rt = env
    lens = [37, 150, 64]
    prompts = _prompts(cfg, lens, n_speech=5)
    speech = torch.randn(3, 5, cfg.llama.hidden) * 0.05
    logits, got_lens = rt.forward_logits(prompts, speech.to(DEV))
    logits = logits.clone()
    assert got_lens == [n + 5 for n in lens]
    ob, of = _llama_oracle(cfg, sd, om.bf16_round), _llama_oracle(cfg, sd)
    off = 0
    for i, segs in enumerate(prompts):
        emb = torch.cat([ob.embed(torch.tensor(segs[0])), speech[i], ob.embed(torch.tensor(segs[2]))])[None]
        emb = emb.to(torch.bfloat16).float() if False else emb
        S = emb.shape[1]
        labels = torch.full((1, S), -100, dtype=torch.long)
        labels[0, -6:] = torch.tensor(segs[2][-6:])
        lb, loss_b = ob.forward(emb, labels)
        lf, _ = of.forward(emb, labels)
        g = logits[off:off + S]
        eb, ef = _rel(g, lb[0]), _rel(g, lf[0])
        print(f"llama logits[{i}] S={S}: rel err vs bf16-rounding oracle {eb:.2e}, vs fp32 oracle {ef:.2e}; "
              f"max abs {float((g.cpu() - lb[0]).abs().max()):.2e} (|logit| max {float(lb.abs().max()):.2f})")
        assert eb < TOL_LOGITS_REL and ef < 1.2e-2   # measured: 2.4e-3 / 5.7e-3 (two-term bf16 P in the D = 128 attention)
        shifted = torch.full((S,), -100, dtype=torch.int32)
        shifted[:-1] = labels[0, 1:].to(torch.int32)
        loss = rt.cross_entropy(g, shifted).cpu()
        assert abs(float(loss) - float(loss_b)) < 2e-3 * max(1.0, abs(float(loss_b)))
        off += S


# asserted bounds = ~2x the values measured on MI355X (printed by the tests)
TOL_LOGITS_REL = 5e-3        # packed prefill / decode logits vs the bf16-rounding oracle, relative L2 per row (measured 2.4e-3 / 3.4e-3)


def test_llama_generate_matches_oracle(env):
    """All 10 greedy decisions, not just the first: the oracle is teacher-forced along the GPU's own tokens (so one numerical
    coin flip cannot make the two paths diverge) and EVERY GPU choice must be the oracle's arg-max up to the measured logit
    error of that step; wherever the oracle's top-1 margin exceeds 4x that error the ids must be identical."""
    from oracle import models as om
    cfg, sd, rt = env
    lens = [33, 90, 61, 12]
    prompts = _prompts(cfg, lens, seed=7)
    res = rt.generate(prompts, None, max_new_tokens=10, suppress_eos=True, want_first_logits=True, want_step_logits=True)
    assert res.tokens.shape == (4, 10) and torch.equal(res.step_logits[0], res.first_logits)
    ob = _llama_oracle(cfg, sd, om.bf16_round)
    decisive = exact = 0
    worst_rel = worst_abs = 0.0
    for i, segs in enumerate(prompts):
        emb = ob.embed(torch.tensor(segs[0]))[None]
        toks = res.tokens[i]
        tf = ob.teacher_forced_logits(emb, toks[None])[0]            # [10, V]
        g = res.step_logits[:, i].cpu()
        for t in range(10):
            err = float((g[t] - tf[t]).abs().max())
            rel = float((g[t] - tf[t]).norm() / tf[t].norm())
            worst_rel, worst_abs = max(worst_rel, rel), max(worst_abs, err)
            top2 = tf[t].topk(2)
            margin = float(top2.values[0] - top2.values[1])
            chosen = int(toks[t])
            assert float(top2.values[0] - tf[t, chosen]) <= 2 * err + 1e-6, (i, t, chosen, int(top2.indices[0]), err, margin)
            assert int(g[t].argmax()) == chosen                       # the argmax kernel agrees with its own logits
            if margin > 4 * err:
                decisive += 1
                assert chosen == int(top2.indices[0]), (i, t)
            exact += int(chosen == int(top2.indices[0]))
        ids = ob.generate_greedy(emb, 10, -1, cfg.llama.pad_id)[0].tolist()
        print(f"generate[{i}]: gpu {toks.tolist()} oracle-free-running {ids}")
    print(f"teacher-forced 10-token check: {exact}/40 decisions equal the oracle arg-max ({decisive} decisive at 4x error), "
          f"step-logit rel-L2 max {worst_rel:.2e}, max abs {worst_abs:.2e}")
    assert worst_rel < TOL_LOGITS_REL
    assert decisive >= 30 and exact >= 38


def test_generate_eos_and_pad_semantics(env):
    """EOS at step 0 -> width-1 output; a row finishing early is filled with pad."""
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    from oracle import models as om
    cfg = SalmonnCfg.tiny(use_beats=False, lora=False)
    sd = synth.salmonn_state(cfg, seed=3, jitter=True, parts=("llama",))
    # force EOS: make the EOS row of lm_head dominate for every hidden state by aligning it with the final norm gain
    lm = sd["llama_model.lm_head.weight"]
    prompts = _prompts(cfg, [20, 31], seed=5)
    rt = SalmonnRuntime(cfg, dict(sd), device=DEV, parts=("llama",))
    base = rt.generate(prompts, None, max_new_tokens=6)
    # pick the token row 0 emits at step 2 and declare it to be EOS: row 0 must then stop there and be pad-filled
    eos = int(base.tokens[0, 2])
    res = rt.generate(prompts, None, max_new_tokens=6, eos_id=eos, pad_id=cfg.llama.pad_id)
    row0 = res.tokens[0].tolist()
    first = row0.index(eos)
    assert all(t == cfg.llama.pad_id for t in row0[first + 1:])
    lsd = {k[len("llama_model."):]: v for k, v in sd.items()}
    ob = om.LlamaOracle(lsd, cfg.llama.n_heads, cfg.llama.rms_eps, rnd=om.bf16_round)
    embs = [ob.embed(torch.tensor(p[0]))[None] for p in prompts]
    # oracle semantics on the same ids: width = longest row, pad after EOS
    exp_w = 0
    for i, e in enumerate(embs):
        ids = ob.generate_greedy(e, 6, eos, cfg.llama.pad_id)
        exp_w = max(exp_w, ids.shape[1])
    assert res.tokens.shape[1] <= 6 and res.tokens.shape[1] >= first + 1
    # EOS at step 0 for every row -> width 1
    eos0 = int(base.tokens[0, 0])
    res1 = rt.generate(prompts[:1], None, max_new_tokens=6, eos_id=eos0)
    assert res1.tokens.shape == (1, 1) and int(res1.tokens[0, 0]) == eos0
    # HF's list form of eos_token_id (Qwen2-Audio's generation_config names two): either id ends its row
    pair = (int(base.tokens[0, 3]), int(base.tokens[1, 1]))
    res2 = rt.generate(prompts, None, max_new_tokens=6, eos_id=pair, pad_id=cfg.llama.pad_id)
    want = [ob.generate_greedy(e, 6, list(pair), cfg.llama.pad_id)[0].tolist() for e in embs]
    width = max(len(w) for w in want)
    assert res2.tokens.shape[1] == width
    for i, w in enumerate(want):
        assert res2.tokens[i, :len(w)].tolist() == w and all(t == cfg.llama.pad_id for t in res2.tokens[i, len(w):].tolist())


def test_decode_graph_replay_matches_eager(env):
    """The HIP-graph replay of the decode loop (2nd+ call with the same batch shape) returns the eager tokens, also when
    the prompt CONTENT (hence positions / cache contents) changes between replays."""
    cfg, sd, rt = env
    rt._graphs.clear(); rt._graph_warm.clear()
    lens = [21, 40, 33]
    outs = []
    for seed in (11, 12, 13, 11):
        res = rt.generate(_prompts(cfg, lens, seed=seed), None, max_new_tokens=8, suppress_eos=True)
        outs.append(res.tokens.clone())
    assert len(rt._graphs) == 1                       # captured on the 2nd call, replayed on the 3rd and 4th
    assert torch.equal(outs[0], outs[3])              # same prompts: eager (1st) == graph replay (4th)
    rt.use_graphs = False
    try:
        eager = rt.generate(_prompts(cfg, lens, seed=13), None, max_new_tokens=8, suppress_eos=True).tokens
    finally:
        rt.use_graphs = True
    assert torch.equal(eager, outs[2])


@pytest.mark.parametrize("n", [72, 20, 5])
def test_decode_on_packed_weights_matches_row_major_path(env, n):
    """Decode GEMMs stream decode-packed weight copies: micro-batch 72 on the 128-row decode tile, 20 on its 64-row variant,
    5 on the skinny kernel.  The same batch on the row-major paths (64x64 split-K / skinny) must give the same greedy
    tokens — the tiles differ only in f32 summation order (the skinny kernel not at all), so at most a numerical coin flip
    or two over n x 6 decisions."""
    cfg, sd, rt = env
    rng = np.random.default_rng(5)
    prompts = _prompts(cfg, rng.integers(9, 40, n).tolist(), seed=300)
    assert rt.llama.decode_packed_weights
    got = rt.generate(prompts, None, max_new_tokens=6, suppress_eos=True).tokens.cpu()
    assert all(L.decode_packed is not None for L in rt.llama.w.layers)
    rt.llama.decode_packed_weights = False
    rt._graphs.clear(); rt._graph_warm.clear()
    try:
        ref = rt.generate(prompts, None, max_new_tokens=6, suppress_eos=True).tokens.cpu()
    finally:
        rt.llama.decode_packed_weights = True
        rt._graphs.clear(); rt._graph_warm.clear()
    same = int((got == ref).all(dim=1).sum())
    print(f"packed vs row-major decode: {same}/{n} rows identical")
    assert torch.equal(got[:, 0], ref[:, 0])          # token 0 comes from the prefill
    assert same >= n - 3 and (n > 8 or same == n)


def test_generate_sampled_and_penalised_greedy(env):
    """f4 generation variants on the full decode path: (a) do_sample with seeded uniforms — the kernel's kept distribution at
    step 0 equals the oracle's filter applied to the SAME logits, draws are reproducible for a seed and replay identically
    from the HIP graph; (b) greedy search under a repetition penalty equals the oracle's penalised greedy search wherever
    the decision is not a numerical coin flip."""
    from oracle import models as om
    cfg, sd, rt = env
    rt._graphs.clear(); rt._graph_warm.clear()
    lens = [25, 47, 30]
    prompts = _prompts(cfg, lens, seed=11)
    V = cfg.llama.vocab
    dbg = (torch.full((3, 1024), -1, dtype=torch.int32, device=DEV), torch.zeros(3, 1024, device=DEV),
           torch.zeros(3, dtype=torch.int32, device=DEV))
    runs = []
    for _ in range(3):          # eager, capture, replay
        gen = torch.Generator(device=DEV).manual_seed(1234)
        res = rt.generate(prompts, None, max_new_tokens=8, do_sample=True, temperature=0.8, top_p=0.9, top_k=50,
                          repetition_penalty=1.2, generator=gen, want_first_logits=True, suppress_eos=True, sample_debug=dbg)
        runs.append(res.tokens.clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert any(k[5] is not None for k in rt._graphs)          # the sampled loop was captured under its own key
    uni = rt.ws.get("gen_uniform", (8, 3), torch.float32).cpu()
    for b in range(3):
        oi, op = om.sample_filter(res.first_logits[b].cpu().numpy(), [], 1.2, 0.8, 50, 0.9)
        n = int(dbg[2][b])
        assert dbg[0][b, :n].tolist() == oi.tolist()
        assert float((dbg[1][b, :n].cpu() - torch.from_numpy(op)).abs().max()) < 1e-6
        cdf = np.cumsum(op.astype(np.float64))
        if np.abs(cdf - float(uni[0, b])).min() > 1e-5:
            assert int(runs[0][b, 0]) == int(oi[om.sample_pick(op, float(uni[0, b]))])
    other = rt.generate(prompts, None, max_new_tokens=8, do_sample=True, temperature=0.8, top_p=0.9, repetition_penalty=1.2,
                        generator=torch.Generator(device=DEV).manual_seed(99), suppress_eos=True).tokens
    assert not torch.equal(other, runs[0])
    # two EOS ids in sample mode (Qwen2-Audio's generation_config: do_sample + [151645, 151643]): same draws, a row ends at the first
    # occurrence of either id and is pad-filled
    pair = (int(runs[0][0, 2]), int(runs[0][1, 4]))
    stop = rt.generate(prompts, None, max_new_tokens=8, do_sample=True, temperature=0.8, top_p=0.9, top_k=50, repetition_penalty=1.2,
                       generator=torch.Generator(device=DEV).manual_seed(1234), eos_id=pair, pad_id=cfg.llama.pad_id).tokens
    for b in range(3):
        want = runs[0][b].tolist()
        cut = next((i for i, t in enumerate(want) if t in pair), None)
        exp = want if cut is None else want[:cut + 1] + [cfg.llama.pad_id] * (len(want) - cut - 1)
        assert stop[b].tolist() == exp[:stop.shape[1]], (b, stop[b].tolist(), exp)
    # (b) penalised greedy vs oracle
    pen = rt.generate(prompts, None, max_new_tokens=8, repetition_penalty=1.5, suppress_eos=True, want_first_logits=True)
    plain = rt.generate(prompts, None, max_new_tokens=8, suppress_eos=True)
    ob = _llama_oracle(cfg, sd, om.bf16_round)
    for b, segs in enumerate(prompts):
        # near-degenerate logits make free-running trajectories diverge on numerical coin flips, so the oracle is driven
        # along the GPU's own tokens and every GPU choice must be (within the logit tolerance) the penalised arg-max
        emb = ob.embed(torch.tensor(segs[0]))[None]
        got = pen.tokens[b].tolist()
        assert got[0] == int(plain.tokens[b, 0])                 # nothing to penalise at step 0
        cache: list = []
        T = emb.shape[1]
        lg = ob.logits(ob.forward_hidden(emb, torch.arange(T)[None], cache)[:, -1:])[0, 0]
        for step, tok in enumerate(got):
            x = lg.clone()
            for t in set(got[:step]):
                x[t] = x[t] * 1.5 if x[t] < 0 else x[t] / 1.5
            tol = 5e-3 * max(1.0, float(lg.abs().max()))
            assert float(x.max() - x[tok]) <= tol, (b, step, float(x.max() - x[tok]), tol)
            if step + 1 < len(got):
                lg = ob.logits(ob.forward_hidden(ob.embed(torch.tensor([tok]))[:, None], torch.full((1, 1), T + step), cache))[0, 0]
        ids, _ = ob.generate_sampled(emb, 3, -1, cfg.llama.pad_id, None, do_sample=False, repetition_penalty=1.5)
        assert ids.shape == (1, 3)


def test_generate_with_chunked_prefill_is_bit_identical(env):
    """generate() prefills at most ``prefill_chunk`` sequences at a time into their own block of the one KV cache and decodes all
    of them together: first-step logits and every token equal the single-pass result, for chunk sizes that divide the batch and
    that leave a ragged last chunk."""
    cfg, sd, rt = env
    lens = [37, 64, 5, 50, 21, 44, 9]
    prompts = _prompts(cfg, lens, seed=4100)
    keep = rt.prefill_chunk
    try:
        rt.prefill_chunk = 128
        want = rt.generate(prompts, None, max_new_tokens=6, suppress_eos=True, want_first_logits=True)
        want_tok, want_first = want.tokens.clone(), want.first_logits.clone()
        for chunk in (1, 3, 4):
            rt.prefill_chunk = chunk
            got = rt.generate(prompts, None, max_new_tokens=6, suppress_eos=True, want_first_logits=True)
            assert torch.equal(got.first_logits, want_first), f"chunk {chunk}: first-step logits differ"
            assert torch.equal(got.tokens, want_tok), f"chunk {chunk}: tokens differ"
    finally:
        rt.prefill_chunk = keep


def test_workspace_stays_bounded_over_ragged_batches(env):
    """a dataset run sees a new total row count on almost every batch.  60 ragged batches (distinct packed
    row totals, batch sizes 1..6, audio 1..4 s) after one largest-shape call must not grow the workspace by a byte, must not
    move a buffer (generation constant), and must leave results bit-identical to the first time a batch was seen."""
    cfg, sd, rt = env
    rng = np.random.default_rng(77)
    big = _prompts(cfg, [64] * 6, seed=900)
    wav_big = _wavs([64000] * 6)
    rt.encode_speech(wav_big, [64000] * 6)
    rt.generate(big, None, max_new_tokens=6, suppress_eos=True)
    rt.forward_logits(big, None)
    probe = _prompts(cfg, [33, 12, 50], seed=901)
    want = rt.generate(probe, None, max_new_tokens=6, suppress_eos=True, want_first_logits=True)
    want_tok, want_first = want.tokens.clone(), want.first_logits.clone()
    probe_wav = _wavs([30000, 47000])
    want_emb = rt.encode_speech(probe_wav, [30000, 47000]).clone()
    bytes0, gen0 = rt.ws.nbytes(), rt.ws.generation
    totals = set()
    for it in range(60):
        b = int(rng.integers(1, 7))
        lens = rng.integers(5, 65, b).tolist()
        totals.add(sum(lens))
        rt.generate(_prompts(cfg, lens, seed=1000 + it), None, max_new_tokens=int(rng.integers(2, 7)), suppress_eos=True)
        wl = rng.integers(16000, 64001, int(rng.integers(1, 7))).tolist()
        rt.encode_speech(_wavs(wl), wl)
        if it % 10 == 0:
            rt.forward_logits(_prompts(cfg, lens, seed=2000 + it), None)
    assert len(totals) >= 40
    assert rt.ws.nbytes() == bytes0, f"workspace grew from {bytes0} to {rt.ws.nbytes()} bytes over ragged batches"
    assert rt.ws.generation == gen0
    assert len(rt._graphs) <= rt.MAX_GRAPHS
    again = rt.generate(probe, None, max_new_tokens=6, suppress_eos=True, want_first_logits=True)
    assert torch.equal(again.tokens, want_tok) and torch.equal(again.first_logits, want_first)
    assert torch.equal(rt.encode_speech(probe_wav, [30000, 47000]), want_emb)


def _beam_replay(dbg, Bn, K, T, eos, lp, pad, pen=1.0):
    """The oracle's scorer driven by the logits the GPU search itself scored, step by step."""
    from oracle import models as om
    bk = om.BeamBookkeeping(Bn, K, T, eos, lp, pen)
    steps = []
    for s, lg in enumerate(dbg["logits"]):
        lg = lg.cpu()
        if lg.shape[0] == Bn:
            lg = lg.repeat_interleave(K, 0)
        parents, toks = bk.step(lg)
        steps.append((parents, toks))
        if bk.done:
            break
    return bk, steps


@pytest.mark.parametrize("K,lp,eos_from", [(3, 1.0, None), (4, 1.0, (0, 2)), (2, 0.0, (1, 1)), (4, 2.0, (2, 3)), (3, -1.0, (0, 1)),
                                           (1, 1.0, None), (3, 1.0, ((0, 2), (1, 1))), (2, -1.0, ((2, 1), (0, 3)))])
@pytest.mark.parametrize("pen", [1.0, 1.4])
def test_beam_search_matches_oracle(env, K, lp, eos_from, pen):
    """num_beams > 1 (models/custom_salmon.py:709-714 -> HF _beam_search).  Three checks on ragged prompts:
    (1) the oracle's scorer replayed on the logits the GPU search scored reproduces the GPU's choices at every step (parents,
        tokens) and its answer — the device bookkeeping is HF's;
    (2) those logits are the model's: every running beam's logits equal the bf16-rounding oracle teacher-forced along that beam's
        history (prompt K/V copied to the beams, generated positions following the parent, decode over rows x K sequences);
    (3) the free-running oracle finds the same hypothesis wherever no decision inside the 2K window was closer than the logit error."""
    from oracle import models as om
    cfg, sd, rt = env
    lens = [33, 90, 12]
    T = 6
    prompts = _prompts(cfg, lens, seed=17)
    pad = cfg.llama.pad_id
    eos = -1
    if eos_from is not None:            # an EOS some hypothesis meets: the token the unconstrained search puts at (row, step)
        free = rt.generate(prompts, None, max_new_tokens=T, suppress_eos=True, num_beams=K, length_penalty=lp, repetition_penalty=pen)
        if isinstance(eos_from[0], tuple):          # two EOS ids (HF's list form): 3K continuations per row
            eos = tuple(int(free.tokens[r, t]) for r, t in eos_from)
        else:
            eos = int(free.tokens[eos_from[0], eos_from[1]])
    dbg = {}
    if K == 1:                          # generate() sends one beam down the greedy path; the beam machinery must agree with it
        res = rt._generate_beam(prompts, None, T, eos, pad, 1, lp, True, 64, debug=dbg, repetition_penalty=pen)
    else:
        res = rt.generate(prompts, None, max_new_tokens=T, eos_id=eos, pad_id=pad, num_beams=K, length_penalty=lp,
                          want_first_logits=True, beam_debug=dbg, suppress_eos=eos == -1, repetition_penalty=pen)
    Bn = len(lens)
    assert len(dbg["logits"]) == T and dbg["logits"][0].shape[0] == Bn and dbg["logits"][1].shape[0] == Bn * K
    # (1) bookkeeping replay
    bk, steps = _beam_replay(dbg, Bn, K, T, eos, lp, pad, pen)
    for s, (parents, toks) in enumerate(steps):
        got_par, got_tok = dbg["parent"][s].cpu().long(), dbg["next"][s].cpu().long()
        if s + 1 < T:                           # at the length limit every continuation stops: the running order is arbitrary
            assert torch.equal(got_tok, toks) and torch.equal(got_par, parents), (s, got_tok, toks, got_par, parents)
    want, want_score = bk.result(pad)
    assert res.tokens.tolist() == want.tolist(), (res.tokens, want)
    got_score = dbg["fin_score"][-1][:, 0].cpu()
    assert torch.allclose(got_score, want_score, rtol=1e-5, atol=1e-5), (got_score, want_score)
    # (2) the logits of every running beam, against the oracle teacher-forced along that beam's tokens
    ob = _llama_oracle(cfg, sd, om.bf16_round)
    worst = 0.0
    for b, segs in enumerate(prompts):
        emb = ob.embed(torch.tensor(segs[0]))[None]
        for s in range(1, T):
            hist = dbg["run_seq"][s - 1][b].cpu().long()[:, :s]          # [K, s]: the tokens fed so far
            for k in range(K):
                tf = ob.teacher_forced_logits(emb, torch.cat([hist[k], torch.zeros(1, dtype=torch.long)])[None])[0, s]
                g = dbg["logits"][s][b * K + k].cpu()
                worst = max(worst, float((g - tf).norm() / tf.norm()))
    print(f"beam K={K} lp={lp} eos={eos}: step-logit rel-L2 max over beams {worst:.2e}; answer {res.tokens.tolist()}")
    assert worst < TOL_LOGITS_REL
    # (3) free-running oracle (informative: a near-tie inside the 2K window may legitimately differ)
    embs = [ob.embed(torch.tensor(p[0]))[None] for p in prompts]
    same = 0
    for b, e in enumerate(embs):
        ids = ob.generate_beam(e, T, eos, pad, K, lp, repetition_penalty=pen)[0].tolist()
        g = res.tokens[b].tolist()
        g = g[:len(ids)] if all(t == pad for t in g[len(ids):]) else g
        same += int(g == ids)
    print(f"free-running oracle agrees on {same}/{Bn} rows")
    if K == 1 and pen == 1.0:      # one beam is greedy search (HF's own equivalence): the GPU's greedy path must give the same ids
        greedy = rt.generate(prompts, None, max_new_tokens=T, eos_id=eos, pad_id=pad, suppress_eos=eos == -1)
        assert greedy.tokens.tolist() == res.tokens.tolist()


def test_beam_search_in_row_groups_matches_one_pass(env):
    """rows x beams above the decode tile run in groups of rows: same answers as one pass."""
    cfg, sd, rt = env
    prompts = _prompts(cfg, [20, 41, 33, 17, 25], seed=23)
    one = rt.generate(prompts, None, max_new_tokens=5, suppress_eos=True, num_beams=3)
    old = rt.beam_rows
    try:
        rt.beam_rows = 6            # two rows per pass
        grouped = rt.generate(prompts, None, max_new_tokens=5, suppress_eos=True, num_beams=3, want_first_logits=True)
    finally:
        rt.beam_rows = old
    assert grouped.tokens.tolist() == one.tokens.tolist() and grouped.first_logits.shape[0] == 5
    with pytest.raises(NotImplementedError):
        rt.generate(prompts, None, max_new_tokens=5, num_beams=3, do_sample=True)
    assert rt.generate(prompts, None, max_new_tokens=5, suppress_eos=True, num_beams=3, repetition_penalty=1.3).tokens.shape == (5, 5)


def test_generate_edge_cases(env):
    """The ends of the input domain: a prompt that fills the position table to its last slot, one-token prompts next to it,
    a single new token, and the inputs that must be refused before anything is launched."""
    from icl_speech_text_llm_amd.runtime.salmonn import speech_segment
    from oracle import models as om
    cfg, sd, rt = env
    T = 4
    full = cfg.llama.max_pos - T                       # prompt + new tokens == max_pos exactly (2048: a multiple of the cache step)
    prompts = _prompts(cfg, [full, 1, 65], seed=31)
    res = rt.generate(prompts, None, max_new_tokens=T, suppress_eos=True, want_first_logits=True)
    assert res.tokens.shape == (3, T)
    ob = _llama_oracle(cfg, sd, om.bf16_round)
    for i in (0, 1):                                    # the longest and the shortest row against the oracle (first-step logits)
        emb = ob.embed(torch.tensor(prompts[i][0]))[None]
        _, first = ob.generate_greedy(emb, 1, -1, cfg.llama.pad_id, return_first_logits=True)
        r = _rel(res.first_logits[i], first[0])
        print(f"edge rows: prompt of {len(prompts[i][0])} positions, first-step logits rel {r:.2e}")
        assert r < TOL_LOGITS_REL
    one = rt.generate(prompts[1:], None, max_new_tokens=1, suppress_eos=True)
    assert one.tokens.shape == (2, 1) and one.tokens[:, 0].tolist() == res.tokens[1:, 0].tolist()
    with pytest.raises(ValueError, match="exceed max_pos"):
        rt.generate(_prompts(cfg, [full + 1], seed=31), None, max_new_tokens=T)
    with pytest.raises(ValueError, match="empty prompt"):
        rt.generate([[[]]], None, max_new_tokens=T)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        rt.generate([[[3, cfg.llama.vocab]]], None, max_new_tokens=T)
    with pytest.raises(ValueError, match="speech segment"):
        rt.generate([[[3, 4], speech_segment(0, 5)]], torch.zeros(1, 4, cfg.llama.hidden, device=DEV), max_new_tokens=T)
    with pytest.raises(ValueError, match="num_beams"):
        rt.generate(prompts[1:], None, max_new_tokens=T, num_beams=0)
    with pytest.raises(ValueError, match="num_beams <= 8"):
        rt.generate(prompts[1:], None, max_new_tokens=T, num_beams=9)
    with pytest.raises(ValueError, match="max_new_tokens <= 64"):
        rt.generate(prompts[1:], None, max_new_tokens=65, num_beams=2)
    sampled = rt.generate(prompts[1:], None, max_new_tokens=2, do_sample=True, top_k=100000, top_p=0.9,
                          generator=torch.Generator(device=DEV).manual_seed(1))      # HF clamps top_k to the vocabulary
    assert sampled.tokens.shape[0] == 2
    # top_k = 0 / None is HF's "no top-k filter" (a generation_config.json may say so): it must run, and give the same draws as
    # any top_k >= vocabulary; a top_k between the kernel's candidate-list size and the vocabulary is an ARGUMENT error raised
    # before any launch (ValueError: the CLI logs and skips the batch) — never a device-side IclError (advisor finding, round 3)
    V = cfg.llama.vocab
    outs = [rt.generate(prompts[1:], None, max_new_tokens=3, do_sample=True, top_k=k, top_p=0.8, temperature=0.9,
                        generator=torch.Generator(device=DEV).manual_seed(4)).tokens for k in (0, None, V, 10 * V)]
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    from icl_speech_text_llm_amd.runtime import binding as Bd
    if V > Bd.SAMPLE_TOP_K_MAX + 1:
        with pytest.raises(ValueError, match="top_k"):
            rt.generate(prompts[1:], None, max_new_tokens=3, do_sample=True, top_k=Bd.SAMPLE_TOP_K_MAX + 1)
    with pytest.raises(ValueError, match="top_k"):
        rt.generate(prompts[1:], None, max_new_tokens=3, do_sample=True, top_k=-3)
    with pytest.raises(ValueError, match="sampling knobs"):
        rt.generate(prompts[1:], None, max_new_tokens=3, do_sample=True, temperature=0.0)
    assert rt.generate(prompts[1:], None, max_new_tokens=2, suppress_eos=True).tokens.shape == (2, 2)      # still usable


def test_encode_speech_edge_lengths(env):
    """0.2 s (BEATs' shortest useful clip: 18 fbank frames -> one row of 16x16 patches), exactly 30 s, and more than 30 s in ONE ragged
    batch, each against the oracle run on that clip alone (batch-1 semantics of the reference's CLI).  Past 30 s Whisper's feature
    extractor truncates to 3000 frames while BEATs sees the whole clip, and SALMONN pads the SHORTER stream with zero frames:
    the clip keeps its 1536 BEATs frames and gets 90 windows instead of 88."""
    from oracle import audio_frontend as af, models as om
    cfg, sd, rt = env
    lens = [3200, 480000, 480000 + 12345]
    wav = _wavs(lens)
    got = rt.encode_speech(wav, lens).clone()
    assert rt.last_audio_windows == [88, 88, 90] and got.shape == (3, 90, cfg.llama.hidden) and bool(torch.isfinite(got).all())
    assert float(got[:2, 88:].abs().max()) == 0.0          # rows past an audio's own windows are padding
    for i, n in enumerate(lens):
        spec = torch.from_numpy(af.whisper_logmel(wav[i, :n].numpy()))[None]
        ref_b = om.salmonn_encode_speech(sd, spec, wav[i:i + 1, :n], [n], cfg.whisper.n_heads, rnd=om.bf16_round,
                                         beats_cfg=dict(n_heads=cfg.beats.n_heads), qformer_heads=cfg.qformer.n_heads)
        assert ref_b.shape[1] == rt.last_audio_windows[i]
        eb = _rel(got[i, :ref_b.shape[1]], ref_b[0])
        print(f"encode_speech edge [{n} samples, {ref_b.shape[1]} windows]: rel err vs bf16-rounding oracle {eb:.2e}")
        assert eb < 1.5e-3
    again = rt.encode_speech(wav[:2], lens[:2])             # back to the uniform path: 88 windows, same values
    assert again.shape == (2, 88, cfg.llama.hidden) and torch.equal(again, got[:2, :88])

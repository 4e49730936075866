"""`-m gpu`: size-independent properties at the FULL BASELINE.json C2 shapes (Whisper-large-v2 + BEATs + Llama-2-7B dims,
seeded random bf16 weights), where the CPU oracle is too slow to be the checker:

  * batch invariance (bit-exact): an utterance's speech embeddings and prefill logits do not depend on what else is
    packed in the batch (ragged packing, no padding);
  * causality: logits at position t do not change when the tokens after t change;
  * determinism: two runs give identical token ids; EOS-suppressed generation returns exactly max_new_tokens;
  * K1 closed form: silence -> the analytically known constant log-mel.
"""
import numpy as np
import pytest
import torch

from gpu_support import stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    cfg = SalmonnCfg.llama2_7b()
    sd = synth.salmonn_state(cfg, seed=0, device="cuda", dtype=torch.bfloat16)
    r = SalmonnRuntime(cfg, sd, device="cuda", consume=True)
    del sd
    return r


def _wav(i, n):
    return torch.from_numpy(np.clip(np.random.default_rng(1234 + i).normal(0, 0.1, n), -1, 1).astype(np.float32))


def _ids(i, n):
    return np.random.default_rng(99 + i).integers(3, 32000, n).tolist()


def test_encode_speech_is_batch_invariant(rt):
    lens = [480000, 16000 * 7 + 13, 480000]
    wav = torch.zeros(3, 480000)
    for i, n in enumerate(lens):
        wav[i, :n] = _wav(i, n)
    batch = rt.encode_speech(wav, lens).clone()
    assert batch.shape == (3, 88, 4096) and torch.isfinite(batch).all()
    for i, n in enumerate(lens):
        solo = rt.encode_speech(wav[i:i + 1], [n])
        assert torch.equal(solo[0], batch[i]), f"audio {i} depends on its batch neighbours"


def test_prefill_logits_batch_invariant_and_causal(rt):
    from icl_speech_text_llm_amd.runtime.salmonn import speech_segment
    speech = torch.randn(2, 88, 4096, device="cuda") * 0.02
    a, b = _ids(0, 288), _ids(1, 170)
    pa = [a[:280], speech_segment(0, 88), a[280:]]
    pb = [b[:100], speech_segment(88, 88), b[100:]]
    both, lens = rt.forward_logits([pa, pb], speech)
    both = both.clone()
    assert lens == [376, 258] and torch.isfinite(both).all()
    solo_a, _ = rt.forward_logits([pa], speech)
    assert torch.equal(solo_a, both[:376])                       # bit-exact: packing is per-sequence independent
    # causality: change the LAST 8 tokens of prompt a -> logits of all earlier positions are unchanged
    a2 = a[:280] + [(t + 7) % 31000 + 3 for t in a[280:]]
    alt, _ = rt.forward_logits([[a2[:280], speech_segment(0, 88), a2[280:]]], speech)
    assert torch.equal(alt[:368], both[:368])
    assert not torch.equal(alt[368:], both[368:376])


def test_generate_is_deterministic_and_full_width(rt):
    from icl_speech_text_llm_amd.runtime.salmonn import speech_segment
    speech = torch.randn(1, 88, 4096, device="cuda") * 0.02
    p = [[_ids(5, 280), speech_segment(0, 88), _ids(6, 8)]]
    r1 = rt.generate(p, speech, max_new_tokens=10, suppress_eos=True).tokens
    r2 = rt.generate(p, speech, max_new_tokens=10, suppress_eos=True).tokens
    assert r1.shape == (1, 10) and torch.equal(r1, r2)
    assert int(r1.min()) >= 0 and int(r1.max()) < 32001


def test_beam_search_at_full_size_is_consistent(rt):
    """Llama-2-7B dims (32 layers x 32 heads x 128): one beam through the beam machinery (prompt K/V copied to the beam rows,
    decode over them, device bookkeeping) gives the greedy ids; four beams in one pass and in row groups give the same answer,
    deterministically, and the best hypothesis starts from one of the prompt's four most likely tokens."""
    from icl_speech_text_llm_amd.runtime.salmonn import speech_segment
    speech = torch.randn(3, 88, 4096, device="cuda") * 0.02
    p = [[_ids(5, 280), speech_segment(0, 88), _ids(6, 8)], [_ids(7, 120), speech_segment(88, 88)], [_ids(8, 40), speech_segment(176, 88), _ids(9, 33)],
         [_ids(10, 64)], [_ids(11, 150), speech_segment(0, 88)], [_ids(12, 90)]]
    greedy = rt.generate(p, speech, max_new_tokens=6, suppress_eos=True, want_first_logits=True)
    one = rt._generate_beam(p, speech, 6, -1, rt.lm_cfg.pad_id, 1, 1.0, False, 64)
    assert torch.equal(one.tokens, greedy.tokens)
    b4 = rt.generate(p, speech, max_new_tokens=6, suppress_eos=True, num_beams=4)
    again = rt.generate(p, speech, max_new_tokens=6, suppress_eos=True, num_beams=4)
    assert b4.tokens.shape == (6, 6) and torch.equal(b4.tokens, again.tokens)
    old = rt.beam_rows
    try:
        rt.beam_rows = 12                # three rows per pass: 12 and 24 decode rows both run the decode tile, whose arithmetic per
                                         # row does not depend on the row count (the <= 8-row skinny kernel sums in another order)
        grouped = rt.generate(p, speech, max_new_tokens=6, suppress_eos=True, num_beams=4)
    finally:
        rt.beam_rows = old
    assert torch.equal(grouped.tokens, b4.tokens)
    top4 = greedy.first_logits.topk(4, dim=-1).indices.cpu()
    assert all(int(b4.tokens[i, 0]) in top4[i].tolist() for i in range(6))


def test_logmel_of_silence_is_the_closed_form_constant(rt):
    # all-zero audio: power 0 -> log10(1e-10) = -10 everywhere -> max-8 clamp keeps -10 -> (x+4)/4 = -1.5
    spec = rt.log_mel(torch.zeros(1, 480000), [480000])
    assert torch.all(spec == -1.5)


def test_full_size_chain_matches_bf16_rounding_oracle(rt):
    """VERDICT r1 #1 / ADVICE r1: the 7B-dim chain — the 256x256 tile, the fused RoPE / cache-append epilogue, the decode
    tile on decode-packed weights, the streaming norms, none of which the miniature chain tests select — against the
    oracle with the bf16 rounding hook on ONE C2 utterance, stage by stage (log-mel, Whisper, BEATs, speech embeddings,
    prefill hidden state, first-step logits), then all 10 greedy decisions teacher-forced: every GPU choice must be the
    oracle's arg-max up to the measured logit error.  On the decisive-margin weight set the ids must be IDENTICAL.
    The bounds are bench.PARITY_BOUNDS (~2x the values measured on MI355X); ~90 s of host time."""
    import bench
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    cfg = SalmonnCfg.llama2_7b()
    dev = torch.device("cuda", torch.cuda.current_device())
    sd = synth.salmonn_state(cfg, seed=0, device=dev, dtype=torch.bfloat16)      # the fixture's weights again (same seed, same device)
    host = bench._to_host_f32(sd)
    del sd
    rt7 = rt
    wav, ids = bench.synth_utterances(0, 1, cfg.llama.vocab)
    torch.set_num_threads(bench.host_cores())
    # the pure-fp32 oracle (the reference's CPU behaviour) on the same utterance: stage outputs + first-step logits for the
    # ratio criterion rel(gpu, fp32) <= 1.25 x rel(bf16-rounding oracle, fp32)
    _, _, _, fp32_first, fp32_stages = bench.cpu_utterance(host, cfg, wav[0], ids[0], bench.host_cores())
    par = bench.full_size_parity(cfg, host, rt7, dev, wav[0], ids[0], fp32_stages, fp32_first)
    print("full-size parity:", par)
    assert par["ratio_ok"], {k: v.get("ratio_to_bf16_oracle_distance") for k, v in par["stages"].items()}
    for name in ("whisper", "beats", "encode_speech", "first_step_logits"):
        assert par["stages"][name]["ratio_to_bf16_oracle_distance"] <= bench.PARITY_RATIO, (name, par["stages"][name])
    emb0 = rt7.encode_speech(torch.from_numpy(wav[0])[None], [480000]).clone()[0]
    del host
    torch.cuda.empty_cache()
    for k, v in par["stages"].items():
        assert v["rel_l2"] <= bench.PARITY_BOUNDS[k], (k, v)
    dec = par["decode_steps_teacher_forced"]
    assert dec["gpu_choice_is_oracle_argmax_within_2x_logit_error"] == "10/10", dec
    assert dec["rel_l2_max"] <= bench.PARITY_BOUNDS["decode_step_logits"], dec
    mar = bench.margin_parity(cfg, dev, ids[0], emb0)
    print("margin-weights parity:", mar)
    assert mar["tokens_match"] and mar["designed_successor_chain_matches"], mar
    assert mar["oracle_top1_margin_min"] > 20 * mar["step_logits_max_abs_err"], mar
    assert mar["step_logits_rel_l2_max"] <= bench.PARITY_BOUNDS["margin_step_logits"], mar

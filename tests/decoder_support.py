"""Inputs and criteria that the decoder-level test modules share: seeded prompts, the bit-identity of two generate() results, the
CPU oracle of a decoder, the teacher-forced token criteria, the plugin batches, and the numpy stepper of icl_argmax_fsm.  Not a test
module, and shared with CPU tests: everything here runs on the CPU, only teacher_forced_check() is handed a runtime to drive."""
import math
import os

import numpy as np
import torch

import qknorm_ref as qr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# The two prompt generators draw from different random streams; measured tolerances were taken on each, so both stay bit for bit.
def row_prompts(vocab, lens, seed):
    """One text segment per row, row i from its own stream default_rng(seed + i), ids in [3, vocab - 1)."""
    return [[np.random.default_rng(seed + i).integers(3, vocab - 1, n).tolist()] for i, n in enumerate(lens)]


def stream_prompts(vocab, lens, seed):
    """One text segment per row, all rows from the one stream default_rng(seed), ids in [3, vocab - 2)."""
    rng = np.random.default_rng(seed)
    return [[rng.integers(3, vocab - 2, n).tolist()] for n in lens]


def same_generation(a, b):
    assert torch.equal(a.tokens.cpu(), b.tokens.cpu())
    if a.first_logits is not None:
        assert torch.equal(a.first_logits, b.first_logits)


def llama_oracle(sd, c, prefix="llama_model.", rnd=True):
    """The CPU oracle of decoder config `c` on the weights under `prefix` (QKNormOracle where the config has q/k norms); rnd=False
    leaves out the bf16 rounding between operations."""
    from oracle import models as om
    lsd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    cls = qr.QKNormOracle if c.qk_norm else om.LlamaOracle
    return cls(lsd, c.n_heads, c.rms_eps, c.rope_theta, c.lora_scale, rnd=om.bf16_round if rnd else None, n_kv_heads=c.kv_heads)


def teacher_forced_check(rt, ob, prompts, tag):
    """The criteria of test_llama_generate_matches_oracle: the oracle is teacher-forced along the GPU's own 10 tokens; every GPU
    choice is within 2x that step's logit error of the oracle's arg-max, and equal to it wherever the margin exceeds 4x the error.
    Returns the worst step rel-L2."""
    res = rt.generate(prompts, None, max_new_tokens=10, suppress_eos=True, want_first_logits=True, want_step_logits=True)
    assert res.tokens.shape == (len(prompts), 10) and torch.equal(res.step_logits[0], res.first_logits)
    worst = 0.0
    for i, segs in enumerate(prompts):
        toks = res.tokens[i]
        tf = ob.teacher_forced_logits(ob.embed(torch.tensor(segs[0]))[None], toks[None])[0]
        g = res.step_logits[:, i].cpu()
        for t in range(10):
            err = float((g[t] - tf[t]).abs().max())
            worst = max(worst, float((g[t] - tf[t]).norm() / tf[t].norm()))
            top2 = tf[t].topk(2)
            chosen = int(toks[t])
            assert float(top2.values[0] - tf[t, chosen]) <= 2 * err + 1e-6, (tag, i, t, chosen, int(top2.indices[0]), err)
            assert int(g[t].argmax()) == chosen
            if float(top2.values[0] - top2.values[1]) > 4 * err:
                assert chosen == int(top2.indices[0]), (tag, i, t)
    return worst


def salmonn_batch(model, fewshot_mode, input_mode="speech_only", n=2, bs=2, num_examples=2, secs=3.0, vary=True):
    """The first collated batch of the synthetic VoxCeleb items, as the SALMONN plugin's processor builds it."""
    from torch.utils.data import DataLoader
    from icl_speech_text_llm_amd.data.model_processors import get_processor
    from icl_speech_text_llm_amd.data.synthetic_dataset import SyntheticICLDataset
    from icl_speech_text_llm_amd.data.task_configs import DatasetType
    proc = get_processor("salmonn", model.input_processor, model.llama_tokenizer)
    ds = SyntheticICLDataset(proc, [DatasetType.VOXCELEB], n_items=n, fewshot_mode=fewshot_mode, input_mode=input_mode,
                             audio_seconds=secs, num_examples=num_examples, vary_length=vary)
    return next(iter(DataLoader(ds, batch_size=bs, collate_fn=proc.collate_batch)))


def qwen_chat_batch(model, secs=(2.5, 7.0)):
    """(processor output of a one-shot chat with the answer appended, prompt length, the two seeded clips) of the Qwen2-Audio plugin."""
    p = model.input_processor
    audios = [np.clip(np.random.default_rng(10 + i).normal(0, 0.1, int(16000 * s)), -1, 1).astype(np.float32) for i, s in enumerate(secs)]
    conv = [{"role": "system", "content": "Classify the sentiment."},
            {"role": "user", "content": [{"type": "text", "text": "Here are few examples to learn from:\n"},
                                         {"type": "audio", "audio_url": "x"}, {"type": "text", "text": "Label: positive\n"},
                                         {"type": "text", "text": "\nNow analyze this input:\n"}, {"type": "audio", "audio_url": "y"}]}]
    text = p.apply_chat_template(conv, add_generation_prompt=True, tokenize=False)
    enc = p(text=text + "negative<|im_end|>", audios=audios, return_tensors="pt", sampling_rate=16000)
    prompt_len = p(text=text, audios=audios).input_ids.shape[1]
    return enc, prompt_len, audios


# ---- the yardstick: one step of icl_argmax_fsm in plain numpy, following include/icl_hip.h literally --------------------------
def fsm_step_reference(row, state, steps_left, auto):
    """(logits row f32 [V], state, steps_left, automaton) -> (token, next state, log-prob as f64) of an UNFINISHED row.
    ``auto`` needs ``state_off`` / ``edge_tok`` / ``edge_next`` / ``state_dist`` (int sequences) and ``n_states``."""
    row = np.asarray(row, dtype=np.float32)
    off, etok, enext, dist = (np.asarray(x).astype(np.int64) for x in (auto.state_off, auto.edge_tok, auto.edge_next, auto.state_dist))
    with np.errstate(all="ignore"):
        if not 0 <= state < auto.n_states:                    # free row (-1), or a corrupt id handled as free
            ok = ~np.isnan(row)
            if not ok.any():
                return 0, state, float("nan")
            x = np.where(ok, row, -np.inf).astype(np.float64)
            tok = int(np.argmax(x))                           # first index of the maximum
            m = x[tok]
            lp = (x[tok] - m) - math.log(np.exp(x[ok] - m).sum()) if np.isfinite(m) else float("nan")
            return tok, state, lp
        cand = [e for e in range(off[state], off[state + 1]) if dist[enext[e]] <= steps_left - 1]
        assert cand, "the budget precondition steps_left >= state_dist[state] is the caller's"
        x = np.array([row[etok[e]] for e in cand], dtype=np.float64)
        x[np.isnan(x)] = -np.inf
        k = int(np.argmax(x))                                 # edges are sorted by token id: first maximum = lowest token id
        m = x[k]
        lp = (x[k] - m) - math.log(np.exp(x - m).sum()) if np.isfinite(m) else float("nan")
        return int(etok[cand[k]]), int(enext[cand[k]]), lp

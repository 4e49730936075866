"""`-m gpu`: opt-in label-constrained greedy decoding — the ``icl_argmax_fsm`` kernel against the numpy stepper of
tests/decoder_support.py (integer results exact; log-probabilities within 1e-5 * max(1, |lp|) of the stepper's f64 value on the
same f32 logits: f32 epsilon is 6e-8 and a value is a subtraction, one exp and one add per candidate and one log, so a few 1e-7
relative is expected, up to ~1e-6 for a free row's 32 001 - 156 032-term sum with per-lane partial sums; 1e-5 leaves a margin of
about ten and still catches a missing max-subtraction or a wrong candidate set, which cost >= 1e-2), and the runtime / plugin /
CLI path at miniature dims with random weights, where the unconstrained model emits non-labels."""
import json
import math
import os

import numpy as np
import pytest
import torch

from decoder_support import GOLDEN as G, fsm_step_reference, qwen_chat_batch, row_prompts, salmonn_batch
from gpu_support import DEV, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
EOS, PAD = 2, 400


@pytest.fixture(scope="module")
def spm():
    from icl_speech_text_llm_amd.utils.tokenization import load_llama_tokenizer
    return load_llama_tokenizer(os.path.join(G, "llama_spm"), 401)


@pytest.fixture(scope="module")
def auto(spm):
    from icl_speech_text_llm_amd.data.task_configs import DatasetType
    from icl_speech_text_llm_amd.runtime.constraints import build_label_automaton
    return build_label_automaton(spm, list(DatasetType))          # every typed task concatenated, free types at -1


def _close(got, want):
    if math.isnan(want):
        return math.isnan(got)
    return abs(got - want) <= 1e-5 * max(1.0, abs(want))


def _reachable_state(a, rng, steps_left):
    """A state some walk from a start state reaches and that the budget rule allows at ``steps_left`` (the caller's precondition:
    steps_left >= state_dist[state])."""
    starts = [s for s in a.starts.values() if s >= 0 and a.min_tokens(s) <= steps_left]
    s = starts[int(rng.integers(len(starts)))]
    for _ in range(int(rng.integers(0, 7))):
        e = [n for t, n in a.edges(s) if t != a.eos_id and a.min_tokens(n) <= steps_left]
        if not e:
            break
        s = e[int(rng.integers(len(e)))]
    return s


def _kernel_case(a, B, V, seed, steps_left=10):
    """Random logits and row states with every special case of the contract planted in some rows."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, V, generator=g, dtype=torch.float32) * 3.0
    state = np.empty(B, np.int32)
    fin = np.zeros(B, np.int32)
    for b in range(B):
        kind = b % 8 if B >= 8 else (seed + b) % 8
        s = _reachable_state(a, rng, steps_left)
        state[b] = s
        cand_toks = [t for t, _ in a.candidates(s, steps_left)]
        if kind == 1:
            state[b] = -1                                           # free row
        elif kind == 2:
            fin[b] = 1                                              # finished row (its state must stay untouched)
        elif kind == 3:
            logits[b, cand_toks] = 1.25                             # exact tie among all candidates
        elif kind == 4:
            logits[b, cand_toks[0]] = float("nan")                  # NaN and -inf among the candidates
            logits[b, cand_toks[-1]] = float("-inf")
        elif kind == 5:
            logits[b, cand_toks] = float("-inf")                    # nothing finite: the first candidate, NaN log-prob
            logits[b, cand_toks[len(cand_toks) // 2]] = float("nan")
        elif kind == 6:
            state[b] = a.n_states + 5 if b % 16 < 8 else -7        # corrupt state id: handled as free
            logits[b, int(rng.integers(V))] = float("nan")
        elif kind == 7:
            state[b] = -1                                           # free row with NaN / -inf entries and a tie at the top
            i, j = sorted(int(x) for x in rng.choice(V, 2, replace=False))
            logits[b, i] = logits[b, j] = 40.0
            logits[b, int(rng.integers(V))] = float("nan")
            logits[b, int(rng.integers(V))] = float("-inf")
    return logits, state, fin


@pytest.mark.parametrize("V", [32001, 156032])
@pytest.mark.parametrize("B", [1, 8, 256])
def test_argmax_fsm_matches_the_stepper(auto, B, V):
    import icl_speech_text_llm_amd.runtime.binding as Bd
    a = auto
    tables = a.upload(DEV)
    worst = 0.0
    seeds = range(8) if B == 1 else range(2)
    for seed in seeds:
        for steps_left in ((1, 4, 10) if B == 256 else range(1, 11)):
            logits, state, fin = _kernel_case(a, B, V, 1000 * seed + steps_left, steps_left)
            T, step = 12, 12 - steps_left
            lg = logits.to(DEV)
            st, fn = torch.from_numpy(state.copy()).to(DEV), torch.from_numpy(fin.copy()).to(DEV)
            toks = torch.full((B, T), -9, dtype=torch.int32, device=DEV)
            lps = torch.full((B, T), 7.0, dtype=torch.float32, device=DEV)
            nxt = torch.full((B,), -9, dtype=torch.int32, device=DEV)
            Bd.argmax_fsm(lg, tables, st, steps_left, EOS, PAD, fn, toks, step, nxt, out_logprob=lps)
            fn2, toks2, nxt2 = (torch.from_numpy(fin.copy()).to(DEV), torch.full((B, T), -9, dtype=torch.int32, device=DEV),
                                torch.full((B,), -9, dtype=torch.int32, device=DEV))
            Bd.argmax_eos(lg, EOS, PAD, fn2, toks2, step, nxt2)
            torch.cuda.synchronize()
            st, fn, toks, lps, nxt, toks2 = st.cpu().numpy(), fn.cpu().numpy(), toks.cpu().numpy(), lps.cpu().numpy(), nxt.cpu().numpy(), toks2.cpu().numpy()
            assert (toks[:, [c for c in range(T) if c != step]] == -9).all() and (lps[:, [c for c in range(T) if c != step]] == 7.0).all()
            for b in range(B):
                if fin[b]:
                    want = (PAD, int(state[b]), 0.0, 1)
                else:
                    t, n, lp = fsm_step_reference(logits[b].numpy(), int(state[b]), steps_left, a)
                    want = (t, n, lp, int(t == EOS))
                    if not 0 <= state[b] < a.n_states:
                        assert toks[b, step] == toks2[b, step], (b, "free row differs from icl_argmax_eos")
                got = (int(toks[b, step]), int(st[b]), float(lps[b, step]), int(fn[b]))
                assert got[0] == want[0] and got[1] == want[1] and got[3] == want[3] and int(nxt[b]) == want[0], (B, V, seed, steps_left, b, got, want)
                assert _close(got[2], want[2]), (B, V, seed, steps_left, b, got, want)
                if not math.isnan(want[2]):
                    worst = max(worst, abs(got[2] - want[2]) / max(1.0, abs(want[2])))
    print(f"icl_argmax_fsm B={B} V={V}: max |d logprob| / max(1, |lp|) = {worst:.3e} (bound 1e-5)")


def test_argmax_fsm_without_a_logprob_buffer_and_with_two_eos_ids(auto):
    import icl_speech_text_llm_amd.runtime.binding as Bd
    a, V, B = auto, 32001, 8
    logits, state, fin = _kernel_case(a, B, V, 77)
    fin[:] = 0
    state[:] = a.starts["voxceleb"]
    outs = []
    for eos in (EOS, (7, EOS)):
        st, fn = torch.from_numpy(state.copy()).to(DEV), torch.from_numpy(fin.copy()).to(DEV)
        toks = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
        nxt = torch.zeros((B,), dtype=torch.int32, device=DEV)
        Bd.argmax_fsm(logits.to(DEV), a.upload(DEV), st, 5, eos, PAD, fn, toks, 1, nxt)
        outs.append((st.cpu(), fn.cpu(), toks.cpu(), nxt.cpu()))
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    labels = {_id for _id, _ in a.edges(a.starts["voxceleb"])}
    assert set(outs[0][2][:, 1].tolist()) <= labels and not outs[0][1].any()


def test_argmax_fsm_in_a_captured_graph_replays_like_eager(auto):
    import icl_speech_text_llm_amd.runtime.binding as Bd
    a, V, B, T = auto, 32001, 8, 6
    tables = a.upload(DEV)
    logits, state0, _ = _kernel_case(a, B, V, 5, T)
    state0 = np.where((state0 >= 0) & (state0 < a.n_states), a.starts["hvb"], state0).astype(np.int32)
    state0[1] = -1
    lgs = [(torch.randn(B, V, generator=torch.Generator().manual_seed(50 + t)) * 3).to(DEV) for t in range(T)]
    st = torch.zeros(B, dtype=torch.int32, device=DEV)
    fn = torch.zeros(B, dtype=torch.int32, device=DEV)
    toks = torch.zeros((B, T), dtype=torch.int32, device=DEV)
    lps = torch.zeros((B, T), dtype=torch.float32, device=DEV)
    nxt = torch.zeros(B, dtype=torch.int32, device=DEV)

    def reset():
        st.copy_(torch.from_numpy(state0)); fn.zero_(); toks.fill_(-1); lps.fill_(9.0); nxt.fill_(-1)

    def run():
        for t in range(T):
            Bd.argmax_fsm(lgs[t], tables, st, T - t, EOS, PAD, fn, toks, t, nxt, out_logprob=lps)

    reset(); run(); torch.cuda.synchronize()
    eager = [x.clone() for x in (st, fn, toks, lps, nxt)]
    for b in range(B):                                             # the eager pass itself is a walk the stepper reproduces
        s, done = int(state0[b]), False
        for t in range(T):
            if done:
                assert int(eager[2][b, t]) == PAD
                continue
            tok, s, _ = fsm_step_reference(lgs[t][b].cpu().numpy(), s, T - t, a)
            assert int(eager[2][b, t]) == tok
            done = tok == EOS
        if 0 <= state0[b] < a.n_states:
            assert a.is_accepting(int(eager[0][b]))               # out of budget or EOS: on a complete answer
    g = torch.cuda.CUDAGraph()
    reset(); torch.cuda.synchronize()
    with torch.cuda.graph(g):
        run()
    for _ in range(2):
        reset(); g.replay(); torch.cuda.synchronize()
        for x, y in zip(eager, (st, fn, toks, lps, nxt)):
            assert torch.equal(x, y)


# ---- model level: miniature dims, random weights -------------------------------------------------------------------------------
def _runtime(**kw):
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    cfg = SalmonnCfg.tiny(use_beats=False, lora=False, vocab=401)
    sd = synth.salmonn_state(cfg, seed=3, jitter=True, parts=("llama",))
    return cfg, SalmonnRuntime(cfg, dict(sd), device=DEV, parts=("llama",), **kw)


@pytest.fixture(scope="module")
def env():
    return _runtime()


def _check_against_stepper(res, a, starts, T):
    """The emitted tokens are the constrained arg-max of the logits the GPU itself produced; log-probs within the kernel bound."""
    tokens, lps, logits = res.tokens.numpy(), res.token_logprobs.numpy(), res.step_logits.cpu().numpy()
    worst = 0.0
    for b, s in enumerate(starts):
        done = False
        for t in range(tokens.shape[1]):
            if done:
                assert tokens[b, t] == PAD and lps[b, t] == 0.0, (b, t)
                continue
            tok, s, lp = fsm_step_reference(logits[t, b], s, T - t, a)
            assert tokens[b, t] == tok, (b, t, tokens[b].tolist())
            assert _close(float(lps[b, t]), lp), (b, t, float(lps[b, t]), lp)
            worst = max(worst, abs(float(lps[b, t]) - lp) / max(1.0, abs(lp)))
            done = tok == EOS
        if starts[b] >= 0:
            assert a.accepts(starts[b], tokens[b].tolist()), (b, tokens[b].tolist())
    return worst


def _mixed(a, n):
    kinds = ["voxceleb", "hvb", "sqa", "voxpopuli", "meld_emotion_greek", "hvb_greek", "vp_nel", "voxpopuli_greek"]
    names = [kinds[i % len(kinds)] for i in range(n)]
    return names, [a.starts[k] for k in names]


def test_generate_follows_the_automaton_on_the_logits_the_gpu_produced(env, auto):
    cfg, rt = env
    T, lens = 10, [21, 40, 33, 17, 25, 30, 19, 28, 36, 22, 31]
    names, starts = _mixed(auto, len(lens))
    prompts = row_prompts(cfg.llama.vocab, lens, seed=99)
    free = rt.generate(prompts, None, max_new_tokens=T, eos_id=EOS, pad_id=PAD, want_first_logits=True)
    assert free.token_logprobs is None
    res = rt.generate(prompts, None, max_new_tokens=T, eos_id=EOS, pad_id=PAD, want_first_logits=True, want_step_logits=True,
                      constraint=(auto, starts))
    assert res.token_logprobs.shape == res.tokens.shape and res.token_logprobs.dtype == torch.float32 and not res.token_logprobs.is_cuda
    worst = _check_against_stepper(res, auto, starts, T)
    print(f"generate(constraint): max |d logprob| / max(1, |lp|) = {worst:.3e} (bound 1e-5)")
    assert torch.equal(res.first_logits, free.first_logits)               # prefill untouched: bit-identical
    typed = [b for b, s in enumerate(starts) if s >= 0]
    assert any(not auto.accepts(starts[b], free.tokens[b].tolist()) for b in typed)      # the feature does something
    for b, s in enumerate(starts):
        if s < 0:                                                          # free rows: the unconstrained run's tokens
            w = min(res.tokens.shape[1], free.tokens.shape[1])
            assert torch.equal(res.tokens[b, :w], free.tokens[b, :w]), b


def test_eager_capture_replay_agree_and_a_second_automaton_gets_its_own_graph(env, auto, spm):
    from icl_speech_text_llm_amd.runtime.constraints import LabelAutomaton
    cfg, rt = env
    rt._graphs.clear(); rt._graph_warm.clear()
    T, lens = 10, [21, 40, 33, 18]
    names, starts = _mixed(auto, len(lens))
    prompts = row_prompts(cfg.llama.vocab, lens, seed=7)
    outs = [rt.generate(prompts, None, max_new_tokens=T, eos_id=EOS, pad_id=PAD, constraint=(auto, starts)) for _ in range(3)]
    assert len(rt._graphs) == 1
    assert all(torch.equal(outs[0].tokens, o.tokens) and torch.equal(outs[0].token_logprobs, o.token_logprobs) for o in outs[1:])
    # the same tables with every label token moved up by one id: same shapes, another language
    shifted = LabelAutomaton(auto.state_off, [t if t == EOS else t + 1 for t in auto.edge_tok.tolist()], auto.edge_next, auto.starts,
                             auto.vocab, EOS)
    other = [rt.generate(prompts, None, max_new_tokens=T, eos_id=EOS, pad_id=PAD, constraint=(shifted, starts)) for _ in range(3)]
    assert len(rt._graphs) == 2
    for o in other:
        assert torch.equal(o.tokens, other[0].tokens)
        typed = [b for b, s in enumerate(starts) if s >= 0]
        assert all(shifted.accepts(starts[b], o.tokens[b].tolist()) for b in typed)
        assert not all(auto.accepts(starts[b], o.tokens[b].tolist()) for b in typed)      # ITS language, not the first one's
    again = rt.generate(prompts, None, max_new_tokens=T, eos_id=EOS, pad_id=PAD, constraint=(auto, starts))
    assert torch.equal(again.tokens, outs[0].tokens)


def test_three_tokens_on_hvb_end_on_a_complete_label_list(env, auto):
    cfg, rt = env
    lens = [20, 31, 26, 40, 23, 35]
    s0 = auto.starts["hvb"]
    assert auto.min_tokens(s0) == 3
    prompts = row_prompts(cfg.llama.vocab, lens, seed=3)
    res = rt.generate(prompts, None, max_new_tokens=3, eos_id=EOS, pad_id=PAD, constraint=(auto, [s0] * len(lens)),
                      want_step_logits=True)
    _check_against_stepper(res, auto, [s0] * len(lens), 3)
    for row in res.tokens.tolist():
        assert auto.accepts(s0, row) and len(row) == 3 and EOS not in row[:2]
    with pytest.raises(ValueError, match="shortest answer"):
        rt.generate(prompts, None, max_new_tokens=2, eos_id=EOS, pad_id=PAD, constraint=(auto, [s0] * len(lens)))


def test_fp8_weights_and_fp8_cache_run_constrained(auto):
    cfg, rt = _runtime(llm_weight_dtype="fp8", llm_kv_dtype="fp8")
    T, lens = 10, [21, 40, 33, 17, 25]
    names, starts = _mixed(auto, len(lens))
    prompts = row_prompts(cfg.llama.vocab, lens, seed=99)
    for _ in range(3):                                                      # eager, capture, replay
        res = rt.generate(prompts, None, max_new_tokens=T, eos_id=EOS, pad_id=PAD, want_step_logits=True, constraint=(auto, starts))
        _check_against_stepper(res, auto, starts, T)


def test_qwen_runtime_decodes_constrained():
    from icl_speech_text_llm_amd.data.task_configs import DatasetType as DT
    from icl_speech_text_llm_amd.models.model_factory import ModelFactory
    from icl_speech_text_llm_amd.runtime.constraints import grammar_of
    from icl_speech_text_llm_amd.utils.evaluation_utils import clean_prediction
    m = ModelFactory.create_model("qwen2", device="cuda", arch="tiny", model_path="none").eval()
    m.generation_config["max_new_tokens"] = 24
    enc, prompt_len, _ = qwen_chat_batch(m)
    batch = {"input_ids": enc.input_ids[:, :prompt_len], "attention_mask": enc.attention_mask[:, :prompt_len],
             "input_features": enc.input_features, "feature_attention_mask": enc.feature_attention_mask}
    plain = m.generate_ids(dict(batch), want_first_logits=True)
    for dt in (DT.VOXCELEB, DT.VOXPOPULI):
        res = m.generate_ids(dict(batch, constrain_labels=True, dataset_type=[dt]), want_first_logits=True)
        assert torch.equal(res.first_logits, plain.first_logits) and res.token_logprobs is not None
        text = m.decode_ids(res.tokens)[0]
        ok = set(grammar_of(dt)[1]) | ({"none"} if dt == DT.VOXPOPULI else set())
        assert all(p.strip() in ok for p in text.split(",")) and clean_prediction(text, dt) == text, (dt, text)
    assert plain.token_logprobs is None


# ---- plugin and CLI ----------------------------------------------------------------------------------------------------------
def _valid_answer(text, dataset_type):
    from icl_speech_text_llm_amd.runtime.constraints import grammar_of
    kind, labels = grammar_of(dataset_type)
    parts = [p.strip() for p in text.split(",")]
    if kind == "single":
        return len(parts) == 1 and parts[0] in labels
    return all(p in labels for p in parts) or (kind == "list+none" and parts == ["none"])


def test_plugin_key_constrains_and_its_absence_changes_nothing():
    from icl_speech_text_llm_amd.models.model_factory import ModelFactory
    m = ModelFactory.create_model("salmonn", device="cuda", arch="tiny", low_resource=True, llama_path="none", lora_alpha=32).eval()
    b = salmonn_batch(m, "text", n=4, bs=4)
    b = {k: (v.to("cuda") if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
    b["max_new_tokens"] = 48
    never = m.generate_ids(dict(b), want_first_logits=True)
    off = m.generate_ids(dict(b, constrain_labels=False), want_first_logits=True)
    assert torch.equal(never.tokens, off.tokens) and torch.equal(never.first_logits, off.first_logits) and off.token_logprobs is None
    on = m.generate_ids(dict(b, constrain_labels=True), want_first_logits=True)
    assert torch.equal(on.first_logits, never.first_logits)
    texts = m.decode_ids(on.tokens)
    assert all(_valid_answer(t, dt) for t, dt in zip(texts, b["dataset_type"])), texts
    assert not all(_valid_answer(t, dt) for t, dt in zip(m.decode_ids(never.tokens), b["dataset_type"]))
    assert m.generate_output(dict(b, constrain_labels=True)) == texts


def test_cli_flag_makes_every_typed_prediction_a_valid_answer(tmp_path):
    from icl_speech_text_llm_amd.data import task_configs as tc
    from icl_speech_text_llm_amd.inference.inference import main
    root = tmp_path / "data"
    common = ["--peft_model_path", "", "--run_name", "t", "--dataset_type", "voxceleb-hvb-voxpopuli-meld_emotion_greek", "--arch", "tiny",
              "--device", "cuda", "--dataset_root", str(root), "--write_synthetic_datasets", "--synthetic_items", "5",
              "--num_examples", "2", "--batch_size", "4", "--num_workers", "0", "--max_new_tokens", "48"]
    outs = {}
    try:
        for tag, extra in (("on", ["--constrain_labels", "true"]), ("off", []), ("off2", ["--constrain_labels", "false"])):
            out = tmp_path / tag
            assert main(common + extra + ["--results_dir", str(out)]) == 0
            files = sorted(f for f in os.listdir(out) if f.endswith(("_results.json", "_metrics.json")))
            outs[tag] = {f: open(out / f, "rb").read() for f in files}
    finally:
        tc.set_dataset_root(None)
    assert outs["off"] == outs["off2"]                                      # flag off: the same bytes
    res = json.loads([v for k, v in outs["on"].items() if k.endswith("_results.json")][0])
    assert len(res) == 20
    for r in res:
        assert _valid_answer(r["predicted_label"], r["dataset_type"]), r
        assert r["predicted_label (cleaned)"] == r["predicted_label"], r
    free = json.loads([v for k, v in outs["off"].items() if k.endswith("_results.json")][0])
    assert not all(_valid_answer(r["predicted_label"], r["dataset_type"]) for r in free)

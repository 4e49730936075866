"""CPU: opt-in label-constrained greedy decoding — the automaton builder (runtime/constraints.py), the refusals of
``generate(constraint=...)``, the CLI flag and the ``icl_argmax_fsm`` entry point's surface.  The kernel and the model path are
checked in tests/test_gpu_constrained.py, against ``fsm_step_reference`` of tests/decoder_support.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from decoder_support import GOLDEN as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def all_typed():
    from icl_speech_text_llm_amd.data.task_configs import DatasetType
    from icl_speech_text_llm_amd.runtime.constraints import grammar_of
    return [dt for dt in DatasetType if grammar_of(dt)[0] != "free"]


def tokenizers():
    from icl_speech_text_llm_amd.utils.tokenization import ByteTokenizer, load_llama_tokenizer
    return {"spm": load_llama_tokenizer(os.path.join(G, "llama_spm"), 401), "byte": ByteTokenizer(260)}


@pytest.fixture(scope="module")
def toks():
    return tokenizers()


def _ids(tok, text):
    return [int(t) for t in tok(text, add_special_tokens=False)["input_ids"]]


def _bfs_dist(a):
    """Brute force: for every state, breadth-first search forward until an accepting state is met."""
    out = []
    for s in range(a.n_states):
        seen, frontier, d = {s}, [s], 0
        while True:
            if any(any(t == a.eos_id for t, _ in a.edges(x)) for x in frontier):
                out.append(d)
                break
            nxt = []
            for x in frontier:
                for _, n in a.edges(x):
                    if n not in seen:
                        seen.add(n)
                        nxt.append(n)
            assert nxt, f"state {s} reaches no accepting state"
            frontier, d = nxt, d + 1
    return out


# ---- 1. builder --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["spm", "byte"])
def test_every_accepted_string_of_up_to_three_labels_is_a_word_of_its_automaton(toks, name):
    from icl_speech_text_llm_amd.runtime.constraints import build_label_automaton, grammar_of
    tok = toks[name]
    for dt in all_typed():
        kind, labels = grammar_of(dt)
        a = build_label_automaton(tok, [dt])
        start = a.starts[dt.value]
        assert start == 0 and a.state_dist.tolist() == _bfs_dist(a), dt
        words = list(labels)
        if kind != "single":
            words += [x + ", " + y for x in labels for y in labels]
            words += [x + ", " + y + ", " + z for x in labels for y in labels for z in labels[:4]]
            if kind == "list+none":
                words.append("none")
        for w in words:
            ids = _ids(tok, w)
            assert a.accepts(start, ids) and a.accepts(start, ids + [a.eos_id]), (dt, w)
        # and nothing else of the obvious kind: a truncated label, a list of a single-label type, a foreign word
        bad = [labels[0][:-1], labels[0] + ",", "zzz"] + ([labels[0] + ", " + labels[1]] if kind == "single" else [labels[0] + ", "])
        for w in bad:
            assert not a.accepts(start, _ids(tok, w)), (dt, w)
        for s in range(a.n_states):                           # CSR invariants the kernel relies on
            e = a.edges(s)
            assert e and [t for t, _ in e] == sorted({t for t, _ in e})


@pytest.mark.parametrize("name", ["spm", "byte"])
def test_random_walks_decode_to_exactly_the_labels_walked(toks, name):
    """>= 200 seeded walks per type under the budget rule at max_new_tokens = 10: the text that ``decode_ids`` + ``clean_prediction``
    give is exactly the list of labels walked, each a valid label, none truncated."""
    from icl_speech_text_llm_amd.runtime.constraints import build_label_automaton, grammar_of
    from icl_speech_text_llm_amd.utils.evaluation_utils import clean_prediction
    tok = toks[name]
    T = 10
    for dt in all_typed():
        kind, labels = grammar_of(dt)
        a = build_label_automaton(tok, [dt])
        start = a.starts[dt.value]
        if a.min_tokens(start) > T:                           # e.g. 'positive' is 8 bytes: fits; nothing of this table exceeds 10
            pytest.fail(f"{dt}: shortest answer {a.min_tokens(start)} tokens > {T}")
        rng = np.random.default_rng(sum(map(ord, name + dt.value)))
        lengths = set()
        for _ in range(200):
            s, ids = start, []
            for step in range(T):
                cand = a.candidates(s, T - step)
                assert cand, (dt, s, step)
                t, s = cand[int(rng.integers(len(cand)))]
                ids.append(t)
                if t == a.eos_id:
                    break
            assert a.is_accepting(s), (dt, ids)               # out of budget or EOS: always on a complete answer
            text = tok.batch_decode([ids + [tok.pad_token_id] * (T - len(ids))], skip_special_tokens=True)[0]
            got = clean_prediction(text, dt)
            parts = [p.strip() for p in text.split(",")]
            ok = set(labels) | ({"none"} if kind == "list+none" else set())
            assert all(p in ok for p in parts), (dt, text)
            assert (len(parts) == 1) if kind == "single" else ("none" not in parts or parts == ["none"]), (dt, text)
            assert got == ", ".join(parts), (dt, text, got)
            assert a.accepts(start, _ids(tok, ", ".join(parts))), (dt, text)
            lengths.add(len(parts))
        if dt.value == "hvb" and name == "spm":
            assert max(lengths) >= 2, (dt, lengths)           # the walks do reach lists where ten tokens hold one


def test_a_tokenizer_whose_cut_depends_on_the_neighbour_label_is_refused():
    from icl_speech_text_llm_amd.data.task_configs import DatasetType
    from icl_speech_text_llm_amd.runtime.constraints import build_label_automaton
    from icl_speech_text_llm_amd.utils.tokenization import ByteTokenizer

    class Contextual(ByteTokenizer):
        """Bytes, except that 'law, org' (and only that neighbourhood) merges its separator into one token."""

        def encode(self, text, add_special_tokens=True):
            ids = []
            for i, part in enumerate(text.split("law, org")):
                ids += ([259] if i else []) + super().encode(part, add_special_tokens=False)
            return ids

    with pytest.raises(ValueError, match="depends on the neighbouring label"):
        build_label_automaton(Contextual(300), [DatasetType.VOXPOPULI])
    build_label_automaton(Contextual(300), [DatasetType.VOXCELEB])          # single-label types never meet the merge


def test_the_subword_stand_in_passes_single_labels_and_fails_the_decode_check_on_lists():
    from icl_speech_text_llm_amd.runtime.constraints import build_label_automaton, grammar_of
    from icl_speech_text_llm_amd.utils.tokenization import SubwordStandInTokenizer
    tok = SubwordStandInTokenizer(32001)
    for dt in all_typed():
        if grammar_of(dt)[0] == "single":
            a = build_label_automaton(tok, [dt])
            assert all(a.accepts(0, _ids(tok, l)) for l in grammar_of(dt)[1])
        else:                                                  # its comma-carrying pieces are hashed ids, which decode to nothing
            with pytest.raises(ValueError, match="does not decode"):
                build_label_automaton(tok, [dt])


def test_constructor_validates_what_it_uploads():
    from icl_speech_text_llm_amd.runtime.constraints import LabelAutomaton
    ok = dict(state_off=[0, 1, 2], edge_tok=[5, 2], edge_next=[1, 1], starts={"t": 0}, vocab=10, eos_id=2)
    a = LabelAutomaton(**ok)
    assert a.state_dist.tolist() == [1, 0] and a.state_off.dtype == torch.int32 and a.n_states == 2 and a.n_edges == 2
    for change in (dict(state_off=[0, 2, 1]), dict(state_off=[0, 1, 3]), dict(edge_tok=[10, 2]), dict(edge_tok=[-1, 2]),
                   dict(edge_next=[2, 1]), dict(edge_next=[1, 0]),                      # out of range; EOS edge not a self loop
                   dict(state_off=[0, 2, 2], edge_tok=[5, 5], edge_next=[1, 1]),        # duplicate token in a state
                   dict(state_off=[0, 2, 2], edge_tok=[6, 5], edge_next=[0, 0]),        # unsorted, and nothing accepting
                   dict(edge_tok=[5, 3]),                                               # no state reaches an accepting one
                   dict(starts={"t": 2}), dict(eos_id=10), dict(vocab=0)):
        with pytest.raises(ValueError):
            LabelAutomaton(**dict(ok, **change))


# ---- 2. free types, concatenation ------------------------------------------------------------------------------------------
def test_free_types_and_multi_task_concatenation(toks):
    from icl_speech_text_llm_amd.data.task_configs import DatasetType as DT
    from icl_speech_text_llm_amd.runtime.constraints import build_label_automaton, constraint_for_batch, grammar_of
    tok = toks["spm"]
    a = build_label_automaton(tok, list(DT))
    for dt in DT:
        assert (a.starts[dt.value] == -1) == (grammar_of(dt)[0] == "free")
    for free in (DT.SQA, DT.VOXPOPULI_NEL, DT.VP_NEL, DT.VOXCELEB_SWAP, DT.HVB_SWAP, DT.VOXPOPULI_SWAP, DT.MELD_EMOTION_SWAP):
        assert a.starts[free.value] == -1
    assert a.start_states([DT.HVB, DT.SQA, "voxceleb"]) == [a.starts["hvb"], -1, a.starts["voxceleb"]]
    # each type keeps ITS language: the words of one type are accepted from its start state only
    words = {dt: grammar_of(dt)[1] for dt in all_typed()}
    for dt in all_typed():
        single = build_label_automaton(tok, [dt])
        for other in all_typed():
            for w in words[other] + ([words[other][0] + ", " + words[other][1]] if grammar_of(other)[0] != "single" else []):
                ids = _ids(tok, w)
                assert a.accepts(a.starts[dt.value], ids) == single.accepts(0, ids), (dt, other, w)
    with pytest.raises(ValueError):
        build_label_automaton(tok, [DT.SQA])                   # nothing to constrain
    with pytest.raises(ValueError):
        a2 = build_label_automaton(tok, [DT.HVB])
        a2.start_states([DT.VOXCELEB])
    cache = {}
    assert constraint_for_batch(cache, tok, [DT.SQA, DT.SQA], tok.eos_token_id, len(tok)) is None
    c1 = constraint_for_batch(cache, tok, [DT.HVB, DT.SQA], tok.eos_token_id, len(tok))
    c2 = constraint_for_batch(cache, tok, [DT.SQA, DT.HVB, DT.HVB], tok.eos_token_id, len(tok))
    assert c1[0] is c2[0] and c1[1] == [0, -1] and c2[1] == [-1, 0, 0]      # built once per set of types


# ---- 3. refusals before any device call; CLI ------------------------------------------------------------------------------------
def _cpu_runtime(monkeypatch):
    """A runtime object without a device behind it whose binding fails the test on any call."""
    import icl_speech_text_llm_amd.runtime.binding as B
    from icl_speech_text_llm_amd.runtime import salmonn
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg

    def boom(*a, **k):
        raise AssertionError("a device call was made before the refusal")

    for name in ("argmax_fsm", "argmax_eos", "sample_eos", "embed_gather_interleave", "gather_rows", "gemm", "load_library"):
        monkeypatch.setattr(B, name, boom)
    rt = salmonn.SalmonnRuntime.__new__(salmonn.SalmonnRuntime)
    rt.cfg = SalmonnCfg.tiny(use_beats=False, lora=False)
    rt.lm_cfg, rt.ws, rt.device = rt.cfg.llama, None, torch.device("cpu")
    monkeypatch.setattr(salmonn.CausalLMRuntimeMixin, "embed_prompts", boom)
    return rt


def test_generate_refuses_bad_constraints_with_value_errors_before_any_launch(monkeypatch, toks):
    from icl_speech_text_llm_amd.data.task_configs import DatasetType as DT
    from icl_speech_text_llm_amd.runtime.binding import IclError
    from icl_speech_text_llm_amd.runtime.constraints import build_label_automaton
    rt = _cpu_runtime(monkeypatch)
    a = build_label_automaton(toks["byte"], [DT.VOXCELEB, DT.HVB])
    prompts = [[[5, 6, 7]], [[8, 9]]]
    good = (a, a.start_states([DT.VOXCELEB, DT.HVB]))
    assert a.min_tokens(good[1][0]) == 7                       # 'neutral'
    cases = [dict(max_new_tokens=6), dict(do_sample=True), dict(repetition_penalty=1.2), dict(num_beams=2), dict(suppress_eos=True),
             dict(constraint=(a, [0])), dict(constraint=(a, [0, a.n_states])), dict(constraint=(a, [0, -2])), dict(constraint=a),
             dict(eos_id=7)]
    for kw in cases:
        args = dict(dict(max_new_tokens=10, constraint=good), **kw)
        with pytest.raises(ValueError) as ei:
            rt.generate(prompts, None, **args)
        assert not isinstance(ei.value, IclError), kw
    with pytest.raises(AssertionError, match="device call"):    # a good constraint gets past the checks, to the (stubbed) device
        rt.generate(prompts, None, max_new_tokens=10, constraint=good)
    big = build_label_automaton(toks["spm"], [DT.VOXCELEB])       # 401 ids on a 260-id model
    with pytest.raises(ValueError, match="vocabulary"):
        rt.generate(prompts, None, constraint=(big, [0, 0]))


def test_overlong_drop_hands_the_surviving_rows_start_states_on(monkeypatch, toks):
    from icl_speech_text_llm_amd.data.task_configs import DatasetType as DT
    from icl_speech_text_llm_amd.runtime import salmonn
    from icl_speech_text_llm_amd.runtime.constraints import build_label_automaton
    rt = _cpu_runtime(monkeypatch)
    a = build_label_automaton(toks["byte"], [DT.VOXCELEB, DT.HVB])
    seen = []
    real = salmonn.CausalLMRuntimeMixin._check_constraint

    def spy(self, constraint, n_rows, *rest):
        out = real(self, constraint, n_rows, *rest)
        seen.append((n_rows, list(out[1])))
        return out

    monkeypatch.setattr(salmonn.CausalLMRuntimeMixin, "_check_constraint", spy)
    prompts = [[[5] * 10], [[5] * 2100], [[6] * 12]]              # row 1 is over max_pos
    starts = [a.starts["hvb"], a.starts["voxceleb"], -1]
    with pytest.raises(AssertionError, match="device call"):
        rt.generate(prompts, None, max_new_tokens=10, constraint=(a, starts), overlong="drop")
    assert seen == [(3, starts), (2, [starts[0], starts[2]])]


def test_plugin_reads_the_batch_key_and_needs_the_dataset_type_column():
    from icl_speech_text_llm_amd.data.task_configs import DatasetType as DT
    from icl_speech_text_llm_amd.models.custom_qwen import CustomQwen
    from icl_speech_text_llm_amd.models.model_factory import ModelFactory
    m = ModelFactory.create_model("salmonn", device="cpu", arch="tiny", low_resource=True, llama_path="none")
    assert m._label_constraint({"prompt": ["a", "b"]}) is None and m._label_constraint({"prompt": ["a"], "constrain_labels": False}) is None
    with pytest.raises(ValueError, match="dataset_type"):
        m._label_constraint({"prompt": ["a"], "constrain_labels": True})
    with pytest.raises(ValueError, match="dataset_type"):
        m.generate_ids({"prompt": ["a"], "constrain_labels": True})          # before any launch: this machine has no GPU path
    a, starts = m._label_constraint({"prompt": ["a", "b", "c"], "constrain_labels": True, "dataset_type": [DT.HVB, DT.SQA, DT.MELD]})
    assert starts == [a.starts["hvb"], -1, a.starts["meld"]] and a.vocab == m.cfg.llama.vocab and a.eos_id == m.llama_tokenizer.eos_token_id
    again = m._label_constraint({"prompt": ["a"] * 3, "constrain_labels": True, "dataset_type": [DT.MELD, DT.HVB, DT.SQA]})
    assert again[0] is a                                                         # cached on the plugin
    assert m._label_constraint({"prompt": ["a"], "constrain_labels": True, "dataset_type": [DT.SQA]}) is None
    q = CustomQwen(device="cpu", arch="tiny", model_path="none")
    with pytest.raises(ValueError, match="dataset_type"):
        q.generate_ids({"input_ids": torch.zeros(1, 4, dtype=torch.long), "constrain_labels": True})
    qa, qs = q._label_constraint({"input_ids": torch.zeros(2, 4, dtype=torch.long), "constrain_labels": True,
                                  "dataset_type": [DT.VOXCELEB, DT.VOXPOPULI]}, [q.cfg.llm.eos_id, 7])
    assert qa.eos_id == q.cfg.llm.eos_id and qa.vocab == q.cfg.llm.vocab and qs == [0, qa.starts["voxpopuli"]]


def test_multi_task_wrapper_passes_the_key_through():
    from icl_speech_text_llm_amd.models.multi_task_model import MultiTaskModel
    mt = MultiTaskModel.from_config({"model_type": "salmonn", "device": "cpu", "arch": "tiny", "llama_path": "none",
                                     "task_configs": {"closed": {"constrain_labels": True}, "open": {}}})
    seen = []
    mt.model.generate_output = lambda samples: seen.append(dict(samples)) or []
    mt.generate_output({"prompt": ["x"], "task": ["closed"]})
    mt.generate_output({"prompt": ["x"], "task": ["open"]})
    mt.generate_output({"prompt": ["x"], "task": ["open"], "constrain_labels": True})
    assert seen[0]["constrain_labels"] is True and "constrain_labels" not in seen[1] and seen[2]["constrain_labels"] is True


def test_cli_flag_parses_and_reaches_the_batch_only_when_given(monkeypatch, tmp_path):
    from icl_speech_text_llm_amd.inference import inference as cli
    base = ["--peft_model_path", "", "--run_name", "r", "--dataset_type", "voxceleb", "--arch", "tiny", "--device", "cpu",
            "--synthetic_items", "2", "--batch_size", "2", "--num_workers", "0", "--results_dir", str(tmp_path)]
    assert cli.parse_args(base).constrain_labels is False
    assert cli.parse_args(base + ["--constrain_labels", "true"]).constrain_labels is True
    assert cli.parse_args(base + ["--constrain_labels", "0"]).constrain_labels is False
    from icl_speech_text_llm_amd.models.custom_salmon import CustomSALMONN
    seen = []

    class Stop(Exception):
        pass

    def fake_generate_ids(self, batch, want_first_logits=False):
        seen.append(dict(batch))
        raise Stop

    monkeypatch.setattr(CustomSALMONN, "generate_ids", fake_generate_ids)
    for extra in ([], ["--constrain_labels", "true"]):
        try:
            cli.run_inference(cli.parse_args(base + extra))
        except Exception:                                         # the CLI counts failed batches / wraps failures; the batch was seen
            pass
    assert len(seen) >= 2
    assert "constrain_labels" not in seen[0] and seen[0]["max_new_tokens"] == 10
    assert seen[-1]["constrain_labels"] is True


# ---- 4. entry point ----------------------------------------------------------------------------------------------------------
def test_argmax_fsm_is_declared_bound_and_exported_under_abi_6():
    import icl_speech_text_llm_amd.runtime.binding as b
    header = open(os.path.join(ROOT, "include", "icl_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(icl_\w+)\s*\(", header, flags=re.M))
    assert "icl_argmax_fsm" in declared and "icl_argmax_fsm" in b.EXPORTED_SYMBOLS and callable(b.argmax_fsm)
    assert re.search(r"#define ICL_ABI_VERSION 6\b", header) and b.ABI_VERSION == 6
    lib = b.load_library()
    assert hasattr(lib, "icl_argmax_fsm") and lib.icl_abi_version() == 6
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    assert "icl_argmax_fsm" in set(re.findall(r"\bT\s+(icl_\w+)$", out, flags=re.M))


def test_argmax_fsm_validates_arguments_without_a_gpu():
    import icl_speech_text_llm_amd.runtime.binding as b
    lib = b.load_library()
    P = 4096          # a non-NULL stand-in: every call below must fail its host checks before any launch

    def err(rc, text):
        assert rc == -1 and text.encode() in lib.icl_last_error(), lib.icl_last_error()

    # icl_argmax_fsm(logits, ldl, B, V, state_off, edge_tok, edge_next, state_dist, n_states, n_edges, state, steps_left,
    #                eos_id, eos_id2, pad_id, finished, out_tokens, out_stride, step, next_ids, out_logprob, stream)
    def call(logits=P, ldl=300, B=2, V=260, off=P, tok=P, nxt=P, dist=P, S=4, E=6, state=P, left=3, fin=P, out=P, stride=10, step=0,
             nid=P, lp=None):
        return lib.icl_argmax_fsm(logits, ldl, B, V, off, tok, nxt, dist, S, E, state, left, 2, -1, 259, fin, out, stride, step,
                                  nid, lp, None)

    err(call(logits=None), "icl_argmax_fsm: NULL pointer")
    err(call(state=None), "icl_argmax_fsm: NULL pointer")
    err(call(fin=None), "icl_argmax_fsm: NULL pointer")
    err(call(nid=None), "icl_argmax_fsm: NULL pointer")
    for k in ("off", "tok", "nxt", "dist"):
        err(call(**{k: None}), "NULL automaton table")
    err(call(V=0), "bad sizes")
    err(call(B=0), "bad sizes")
    err(call(ldl=259), "bad sizes")
    err(call(S=0), "empty automaton")
    err(call(E=0), "empty automaton")
    err(call(left=0), "steps_left=0")
    err(call(step=10), "step=10 outside out_stride=10")
    err(call(step=-1), "outside out_stride")

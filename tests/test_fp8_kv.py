"""CPU: the surface of the opt-in FP8 KV cache of the LLM decoder — the plugins' ``llm_kv_dtype`` keyword, the CLI's ``--llm_kv``
flag, the new entry points against the built library and their argument checks (the kernels are checked in
tests/test_gpu_fp8_kv.py)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KV_SYMBOLS = ("icl_kv_append_fp8", "icl_rope_kv_fp8", "icl_attn_decode_fp8", "icl_attn_decode_rope_fp8", "icl_kv_copy_spans_fp8",
              "icl_attn_decode_bf16_epl16")


def test_factory_builds_a_salmonn_with_an_fp8_cache_on_the_cpu():
    from icl_speech_text_llm_amd.models.model_factory import ModelFactory
    m = ModelFactory.create_model("salmonn", device="cpu", arch="tiny", llm_kv_dtype="fp8")
    assert m.llm_kv_dtype == "fp8" and m.salmonn.llm_kv_dtype == "fp8" and m.llm_weight_dtype == "bf16"
    d = ModelFactory.create_model("salmonn", device="cpu", arch="tiny")
    assert d.llm_kv_dtype == "bf16" and d.salmonn.llm_kv_dtype == "bf16"
    both = ModelFactory.create_model("salmonn", device="cpu", arch="tiny", llm_kv_dtype="fp8", llm_weight_dtype="fp8")
    assert both.salmonn.llm_kv_dtype == "fp8" and both.salmonn.llm_weight_dtype == "fp8"


def test_qwen_and_multi_task_pass_the_cache_dtype_through():
    from icl_speech_text_llm_amd.models.custom_qwen import CustomQwen
    from icl_speech_text_llm_amd.models.multi_task_model import MultiTaskModel
    q = CustomQwen(device="cpu", arch="tiny", model_path="none", llm_kv_dtype="fp8")
    assert q.model.llm_kv_dtype == "fp8" and q.model.llm_weight_dtype == "bf16"
    mt = MultiTaskModel.from_config({"model_type": "qwen2", "device": "cpu", "arch": "tiny", "model_path": "none",
                                     "llm_kv_dtype": "fp8"})
    assert mt.model.model.llm_kv_dtype == "fp8"
    ms = MultiTaskModel.from_config({"model_type": "salmonn", "device": "cpu", "arch": "tiny", "llm_kv_dtype": "fp8"})
    assert ms.model.salmonn.llm_kv_dtype == "fp8"


@pytest.mark.parametrize("bad", ["int8", "fp16", "FP8", "e4m3", ""])
def test_unknown_kv_dtype_is_a_value_error(bad):
    from icl_speech_text_llm_amd.models.custom_qwen import CustomQwen
    from icl_speech_text_llm_amd.models.custom_salmon import CustomSALMONN
    from icl_speech_text_llm_amd.models.model_factory import ModelFactory
    from icl_speech_text_llm_amd.runtime.engines import check_kv_dtype
    with pytest.raises(ValueError):
        CustomSALMONN(device="cpu", arch="tiny", llama_path="none", llm_kv_dtype=bad)
    with pytest.raises(ValueError):
        CustomQwen(device="cpu", arch="tiny", model_path="none", llm_kv_dtype=bad)
    with pytest.raises(ValueError):
        check_kv_dtype(bad)
    with pytest.raises(RuntimeError) as ei:           # the factory wraps every failure (reference behaviour), cause kept
        ModelFactory.create_model("salmonn", device="cpu", arch="tiny", llm_kv_dtype=bad)
    assert isinstance(ei.value.__cause__, ValueError)


def test_keyword_comes_after_the_reference_parameters():
    import inspect
    from icl_speech_text_llm_amd.models.custom_qwen import CustomQwen
    from icl_speech_text_llm_amd.models.custom_salmon import CustomSALMONN
    for cls, last_ref in ((CustomSALMONN, "max_txt_len"), (CustomQwen, "use_fp16")):
        params = inspect.signature(cls.__init__).parameters
        names = list(params)
        assert names.index("llm_kv_dtype") > names.index(last_ref)
        assert params["llm_kv_dtype"].default == "bf16"


def test_cli_flag():
    from icl_speech_text_llm_amd.inference.inference import parse_args
    base = ["--peft_model_path", "", "--run_name", "r", "--dataset_type", "voxceleb"]
    assert parse_args(base).llm_kv == "bf16"
    assert parse_args(base + ["--llm_kv", "fp8"]).llm_kv == "fp8"
    with pytest.raises(SystemExit):
        parse_args(base + ["--llm_kv", "int8"])


def test_cli_hands_the_cache_dtype_to_the_factory_only_when_asked(monkeypatch, tmp_path):
    from icl_speech_text_llm_amd.inference import inference as cli
    seen = []

    class Stop(Exception):
        pass

    def fake_create(**kw):
        seen.append(kw)
        raise Stop

    monkeypatch.setattr(cli.ModelFactory, "create_model", staticmethod(fake_create))
    for flag in ("bf16", "fp8"):
        args = cli.parse_args(["--peft_model_path", "", "--run_name", "r", "--dataset_type", "voxceleb", "--device", "cpu",
                               "--results_dir", str(tmp_path), "--llm_kv", flag, "--llm_weights", "fp8"])
        with pytest.raises(RuntimeError) as ei:          # run_inference wraps every failure
            cli.run_inference(args)
        assert isinstance(ei.value.__cause__, Stop)
    assert "llm_kv_dtype" not in seen[0] and seen[1]["llm_kv_dtype"] == "fp8"
    assert seen[0]["llm_weight_dtype"] == seen[1]["llm_weight_dtype"] == "fp8"


def test_kv_entry_points_are_declared_bound_and_exported():
    import icl_speech_text_llm_amd.runtime.binding as b
    header = open(os.path.join(ROOT, "include", "icl_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(icl_\w+)\s*\(", header, flags=re.M))
    assert set(KV_SYMBOLS) <= declared and set(KV_SYMBOLS) <= set(b.EXPORTED_SYMBOLS)
    lib = b.load_library()
    for name in KV_SYMBOLS:
        assert hasattr(lib, name)
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT\s+(icl_\w+)$", out, flags=re.M))
    assert set(KV_SYMBOLS) <= exported


def test_kv_entry_points_validate_arguments_without_a_gpu():
    import icl_speech_text_llm_amd.runtime.binding as b
    lib = b.load_library()
    P = 4096          # a 16-byte-aligned non-NULL stand-in: every call below must fail its host checks before any launch

    def err(rc, text):
        assert rc == -1 and text.encode() in lib.icl_last_error(), lib.icl_last_error()

    # icl_kv_append_fp8(qkv, ld, k_off, v_off, pos, seq_ids, kq, vq, ks, vs, M, H, D, max_len, stream)
    err(lib.icl_kv_append_fp8(None, 384, 128, 256, P, P, P, P, P, P, 1, 2, 64, 8, None), "icl_kv_append_fp8: NULL pointer")
    err(lib.icl_kv_append_fp8(P, 384, 128, 256, P, P, P, P, P, P, 1, 2, 96, 8, None), "head_dim=96")
    err(lib.icl_kv_append_fp8(P, 384, 128, 256, P, P, P, P, P, P, 0, 2, 64, 8, None), "must be > 0")
    err(lib.icl_kv_append_fp8(P + 2, 384, 128, 256, P, P, P, P, P, P, 1, 2, 64, 8, None), "16-byte aligned")
    err(lib.icl_kv_append_fp8(P, 384, 64, 256, P, P, P, P, P, P, 1, 2, 64, 8, None), "disjoint")
    err(lib.icl_kv_append_fp8(P, 384, 128, 256, P, P, P + 8, P, P, P, 1, 2, 64, 8, None), "cache misaligned")
    err(lib.icl_kv_append_fp8(P, 384, 128, 256, P, P, P, P, P + 2, P, 1, 2, 64, 8, None), "cache misaligned")
    # icl_rope_kv_fp8(qkv, ld, k_off, v_off, cos, sin, pos, seq_ids, kq, vq, ks, vs, M, H, D, max_len, stream)
    err(lib.icl_rope_kv_fp8(P, 384, 128, 256, None, P, P, P, P, P, P, P, 1, 2, 64, 8, None), "cos/sin")
    err(lib.icl_rope_kv_fp8(P, 384, 128, 256, P, P, P, None, P, P, P, P, 1, 2, 64, 8, None), "NULL pointer")
    # icl_attn_decode_fp8(Q, ldq, kq, vq, ks, vs, O, ldo, lens, n_seqs, H, D, max_len, scale, stream)
    err(lib.icl_attn_decode_fp8(P, 128, P, P, None, P, P, 128, P, 1, 2, 64, 8, 0.125, None), "icl_attn_decode_fp8: NULL")
    err(lib.icl_attn_decode_fp8(P, 128, P, P, P, P, P, 128, P, 1, 2, 32, 8, 0.125, None), "head_dim=32")
    err(lib.icl_attn_decode_fp8(P, 128, P, P, P, P, P, 128, P, 70000, 2, 64, 8, 0.125, None), "bad sizes")
    err(lib.icl_attn_decode_fp8(P, 128, P + 8, P, P, P, P, 128, P, 1, 2, 64, 8, 0.125, None), "misaligned")
    err(lib.icl_attn_decode_fp8(P, 128, P, P, P, P + 2, P, 128, P, 1, 2, 64, 8, 0.125, None), "misaligned")
    # icl_attn_decode_bf16_epl16(Q, ldq, Kc, Vc, O, ldo, lens, n_seqs, H, D, max_len, scale, stream)
    err(lib.icl_attn_decode_bf16_epl16(P, 128, None, P, P, 128, P, 1, 2, 64, 8, 0.125, None), "NULL pointer")
    err(lib.icl_attn_decode_bf16_epl16(P, 128, P, P, P, 128, P, 1, 2, 96, 8, 0.125, None), "head_dim=96")
    # icl_attn_decode_rope_fp8(qkv, ld, k_off, v_off, cos, sin, pos, seq_ids, kq, vq, ks, vs, O, ldo, lens, n, H, D, T, s, st)
    err(lib.icl_attn_decode_rope_fp8(P, 384, 128, 256, P, P, P, None, P, P, None, P, P, 128, P, 1, 2, 64, 8, 0.125, None),
        "NULL pointer")
    err(lib.icl_attn_decode_rope_fp8(P, 384, 64, 256, P, P, P, None, P, P, P, P, P, 128, P, 1, 2, 64, 8, 0.125, None),
        "disjoint")
    err(lib.icl_attn_decode_rope_fp8(P, 384, 128, 256, P, P, P, None, P, P, P, P + 1, P, 128, P, 1, 2, 64, 8, 0.125, None),
        "misaligned")
    # icl_kv_copy_spans_fp8(src, ssrc, dst, sdst, 6 byte strides, 6 scale strides, 5 id arrays, n_fixed, n_rows, L, H, D,
    #                       src_n_seqs, dst_n_seqs, src_len, dst_len, stream)
    strides = [4096] * 6 + [64] * 6
    err(lib.icl_kv_copy_spans_fp8(P, None, P, P, *strides, None, None, None, None, None, 1, 1, 1, 1, 64, 1, 1, 8, 8, None),
        "NULL pointer")
    err(lib.icl_kv_copy_spans_fp8(P, P, P, P, *strides, None, None, None, None, None, 1, 1, 1, 1, 72, 1, 1, 8, 8, None),
        "multiple of 16")
    err(lib.icl_kv_copy_spans_fp8(P, P, P, P, *([4104] + [4096] * 5 + [64] * 6), None, None, None, None, None, 1, 1, 1, 1, 64,
                                  1, 1, 8, 8, None), "16-byte aligned")
    err(lib.icl_kv_copy_spans_fp8(P, P + 2, P, P, *strides, None, None, None, None, None, 1, 1, 1, 1, 64, 1, 1, 8, 8, None),
        "scale planes misaligned")
    err(lib.icl_kv_copy_spans_fp8(P, P, P, P, *strides, None, None, None, None, None, 1, 2, 1, 1, 64, 1, 1, 8, 8, None),
        "exceeds")

"""CPU: the surface of the opt-in FP8 weight mode of the LLM decoder — the plugins' ``llm_weight_dtype`` keyword, the CLI's
``--llm_weights`` flag and the ABI-6 entry points (the kernels themselves are checked in tests/test_gpu_fp8.py)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP8_SYMBOLS = ("icl_pack_fp8_weights", "icl_gemm_fp8w", "icl_gemm_rmsnorm_fp8w")


def test_factory_builds_a_salmonn_in_fp8_mode_on_the_cpu():
    from icl_speech_text_llm_amd.models.model_factory import ModelFactory
    m = ModelFactory.create_model("salmonn", device="cpu", arch="tiny", llm_weight_dtype="fp8")
    assert m.llm_weight_dtype == "fp8" and m.salmonn.llm_weight_dtype == "fp8"
    d = ModelFactory.create_model("salmonn", device="cpu", arch="tiny")
    assert d.llm_weight_dtype == "bf16" and d.salmonn.llm_weight_dtype == "bf16"


def test_qwen_and_multi_task_pass_the_mode_through():
    from icl_speech_text_llm_amd.models.custom_qwen import CustomQwen
    from icl_speech_text_llm_amd.models.multi_task_model import MultiTaskModel
    q = CustomQwen(device="cpu", arch="tiny", model_path="none", llm_weight_dtype="fp8")
    assert q.model.llm_weight_dtype == "fp8"
    mt = MultiTaskModel.from_config({"model_type": "qwen2", "device": "cpu", "arch": "tiny", "model_path": "none",
                                     "llm_weight_dtype": "fp8"})
    assert mt.model.model.llm_weight_dtype == "fp8"


@pytest.mark.parametrize("bad", ["int8", "fp16", "FP8", ""])
def test_unknown_weight_dtype_is_a_value_error(bad):
    from icl_speech_text_llm_amd.models.custom_qwen import CustomQwen
    from icl_speech_text_llm_amd.models.custom_salmon import CustomSALMONN
    from icl_speech_text_llm_amd.models.model_factory import ModelFactory
    with pytest.raises(ValueError):
        CustomSALMONN(device="cpu", arch="tiny", llama_path="none", llm_weight_dtype=bad)
    with pytest.raises(ValueError):
        CustomQwen(device="cpu", arch="tiny", model_path="none", llm_weight_dtype=bad)
    with pytest.raises(RuntimeError) as ei:           # the factory wraps every failure (reference behaviour), cause kept
        ModelFactory.create_model("salmonn", device="cpu", arch="tiny", llm_weight_dtype=bad)
    assert isinstance(ei.value.__cause__, ValueError)


def test_keyword_comes_after_the_reference_parameters():
    import inspect
    from icl_speech_text_llm_amd.models.custom_qwen import CustomQwen
    from icl_speech_text_llm_amd.models.custom_salmon import CustomSALMONN
    for cls, last_ref in ((CustomSALMONN, "max_txt_len"), (CustomQwen, "use_fp16")):
        names = list(inspect.signature(cls.__init__).parameters)
        assert names.index("llm_weight_dtype") > names.index(last_ref)
        assert inspect.signature(cls.__init__).parameters["llm_weight_dtype"].default == "bf16"


def test_cli_flag():
    from icl_speech_text_llm_amd.inference.inference import parse_args
    base = ["--peft_model_path", "", "--run_name", "r", "--dataset_type", "voxceleb"]
    assert parse_args(base).llm_weights == "bf16"
    assert parse_args(base + ["--llm_weights", "fp8"]).llm_weights == "fp8"
    with pytest.raises(SystemExit):
        parse_args(base + ["--llm_weights", "int8"])


def test_cli_hands_the_mode_to_the_factory_only_when_asked(monkeypatch, tmp_path):
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
                               "--results_dir", str(tmp_path), "--llm_weights", flag])
        with pytest.raises(RuntimeError) as ei:          # run_inference wraps every failure
            cli.run_inference(args)
        assert isinstance(ei.value.__cause__, Stop)
    assert "llm_weight_dtype" not in seen[0] and seen[1]["llm_weight_dtype"] == "fp8"


def test_fp8_entry_points_are_declared_and_exported():
    import icl_speech_text_llm_amd.runtime.binding as b
    header = open(os.path.join(ROOT, "include", "icl_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(icl_\w+)\s*\(", header, flags=re.M))
    assert set(FP8_SYMBOLS) <= declared and set(FP8_SYMBOLS) <= set(b.EXPORTED_SYMBOLS)
    assert re.search(r"#define ICL_ABI_VERSION 6\b", header) and b.ABI_VERSION == 6
    lib = b.load_library()
    assert lib.icl_abi_version() == 6
    for name in FP8_SYMBOLS:
        assert hasattr(lib, name)


def test_fp8_entry_points_validate_arguments_without_a_gpu():
    import ctypes
    import icl_speech_text_llm_amd.runtime.binding as b
    lib = b.load_library()
    assert lib.icl_pack_fp8_weights(None, 64, 16, 64, None, None, None, 64, None) == -1
    assert b"icl_pack_fp8_weights" in lib.icl_last_error()
    g = b.GemmArgs()
    g.A = g.W = g.C = 16
    g.M, g.N, g.K, g.batch, g.split_k, g.lda, g.ldw, g.ldc = 1, 64, 64, 1, 1, 64, 64, 64
    assert lib.icl_gemm_fp8w(ctypes.byref(g), None, None) == -1 and b"w_scale" in lib.icl_last_error()
    g.M = 65
    assert lib.icl_gemm_fp8w(ctypes.byref(g), 16, None) == -1 and b"M <= 64" in lib.icl_last_error()

"""What every module marked `gpu` shares: the device name, the library fixture B, the guard that ends the session after a
device fault, and dev().  Not a test module and not a conftest: a GPU module imports B (where it uses it) and
stop_after_a_device_fault into its own namespace, which is how pytest sees a fixture that lives outside conftest.py
(tests/test_support_layer.py checks that every GPU module does).  Importing this module does not touch CUDA."""
import pytest
import torch

DEV = "cuda"


@pytest.fixture(scope="module")
def B():
    import icl_speech_text_llm_amd.runtime.binding as b
    b.load_library()
    return b


@pytest.fixture(autouse=True)
def stop_after_a_device_fault():
    yield
    if not torch.cuda.is_initialized():     # a test that only spawned processes: the guard must not be what opens the device
        return
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # nothing more may be launched on a faulted device
        pytest.exit(f"device fault: {e}", returncode=3)


def dev(*xs):
    return tuple(x.to(DEV) for x in xs)

"""The launches of the Llama decoder runtime are pinned (no GPU needed): LlamaHIP.prefill / decode_step / logits make the same
library calls, with the same operands, in the same order as when tests/golden/llama_launch_trace.json was written — at real
7B dims, a grouped-query and a head_dim-64 decoder, both weight modes, both KV dtypes, every switch and every batch-size
boundary (tests/tools/launch_trace.py has the matrix and the encoding).  A change to runtime/engines.py that is meant to keep
behaviour keeps these digests; one that is meant to change a launch regenerates the fixture on purpose
(`python tests/tools/launch_trace.py --write`) and says so."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import launch_trace as lt  # noqa: E402


@pytest.fixture(scope="module")
def got():
    if not lt.device_ok():
        pytest.skip(f"the fixture is taken at {lt.N_CU} CUs (MI355X); this device has another count")
    return lt.digests()


def test_matrix_shape():
    """Under 100 groups; the FP8 KV cache is never paired with the grouped-query config."""
    gs = list(lt.groups())
    assert len(gs) == len(set(gs)) == 84
    assert not [g for g in gs if g[0] == "7b_gqa8_bias" and g[2] == "fp8"]
    assert set(lt.load_fixture()) == {"/".join(g) for g in gs}


def test_launch_trace_matches_the_fixture(got):
    want = lt.load_fixture()
    bad = sorted(k for k in want if got.get(k) != want[k])
    assert not bad, f"{len(bad)} of {len(want)} groups launch differently (diff two `launch_trace.py --dump` runs): {bad[:8]}"
    assert set(got) == set(want)


def test_trace_sees_the_routes(got):
    """The digests are not blind: every switch changes its config's trace, as do the weight mode and the KV dtype."""
    for cname in ("7b_lora", "tiny_h4"):
        base = got[f"{cname}/bf16/bf16/default"]
        for sw in lt.SWITCHES:
            if sw == "default" or (cname == "tiny_h4" and sw in ("no_prefill_last_rows", "no_decode_t256")):
                continue        # head_dim 64 never trims the last layer; its GEMMs are too small for the 256 tile's split
            assert got[f"{cname}/bf16/bf16/{sw}"] != base, (cname, sw)
        assert got[f"{cname}/fp8/bf16/default"] != base and got[f"{cname}/bf16/fp8/default"] != base

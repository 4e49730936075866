"""CPU: the segment-to-segment attention flow without a GPU.  (1) The bound of tests/attn_segflow_ref.py is usable and sharp: an
f32 emulation in the kernel's order (64-key tiles, online rescale, hi / lo split, segment sums in key order, row sums in position
order) stays inside it on every case tests/test_gpu_attn_segflow.py runs, and every mutant is rejected on every case that could show
it — causal j < i, key i + 1 admitted, len + 1, flow transposed, ignored query rows / ignored keys counted into segment 0, the
one-hot operand in natural instead of permuted k order, and P rounded once to bf16 (shown by the case whose segments hold single keys
and single rows).  (2) The argument checks of icl_attn_segflow_bf16, called with host pointers or NULL: each refusal returns -1 and
names the argument, before any launch; the runtime's refusals are ``ValueError``s.  (3) ``prompt_attention(want_flow=False)`` makes
exactly today's launches (tests/tools/launch_trace.py, by import), ``want_flow=True`` adds one launch per layer and chunk and keeps
the last layer at full height.  (4) ``AttnReadout.rows`` slices ``flow``.  (5) The symbol is declared and exported, ABI version 6."""
import ctypes
import math
import os
import re
import sys

import pytest
import torch

import attn_segflow_ref as fr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import launch_trace as lt  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def data():
    """Per case: the random inputs, their segments and the float64 reference, computed once."""
    out = {}
    for case in fr.CASES:
        D, H, Hkv, n_seg = case
        q, kc = fr.random_case(fr.LENS, H, Hkv, D)
        seg = fr.make_seg(fr.LENS, n_seg)
        out[case] = (q, kc, seg, fr.reference(q, kc, fr.LENS, seg, n_seg, H, Hkv, D, D ** -0.5))
    return out


def test_cases_cover_the_forms():
    assert {c[0] for c in fr.CASES} == {64, 128} and {c[3] for c in fr.CASES} == {1, 2, 32}
    assert {c[1] // c[2] for c in fr.CASES} == {1, 2, 8} and all(D == 128 for D, H, Hkv, _ in fr.CASES if H != Hkv)
    assert {L % 32 for L in fr.LENS} >= {0, 1, 31} and {L % 64 for L in fr.LENS} >= {0, 1, 63} and {127, 128, 129} <= set(fr.LENS)
    assert sorted(fr.K_PERM) == list(range(16)) and fr.K_PERM[:8] == (0, 1, 2, 3, 8, 9, 10, 11)
    for n_seg in (1, 2, 32):
        seg = fr.make_seg(fr.LENS, n_seg)
        assert bool((seg[:, fr.MAX_LEN - 1] == 0xFF).all())
        used = [set(seg[b, :L].tolist()) for b, L in enumerate(fr.LENS)]
        assert any(any(x >= n_seg for x in u) for u in used), "no ignored id inside a length"


@pytest.mark.parametrize("case", fr.CASES, ids=fr.case_id)
def test_f32_emulation_is_inside_the_bound(data, case):
    D, H, Hkv, n_seg = case
    q, kc, seg, R = data[case]
    flow = fr.emulate_f32(q, kc, fr.LENS, seg, n_seg, H, Hkv, D, D ** -0.5)
    w = fr.worst(flow, R, D)
    print(f"f32 emulation {fr.case_id(case)}: err/bound {w:.3f}")
    assert w <= 1
    empty = (R.N_ac == 0)[:, None].expand_as(flow)
    assert bool((flow[empty] == 0).all())                       # a pair with nothing to count is exactly 0
    # the emulation with the one-hot operand in natural k order is rejected
    bad = fr.emulate_f32(q, kc, fr.LENS, seg, n_seg, H, Hkv, D, D ** -0.5, natural_k_order=True)
    assert fr.worst(bad, R, D) > 1, "the bound admits the natural k order"


# every mutant on every case that could show it: a transposition needs two segments
MUTANT_CASES = [(c, m) for c in fr.CASES for m in fr.REF_MUTANTS if not (m == "transposed" and c[3] == 1)]


@pytest.mark.parametrize("case,mutant", MUTANT_CASES, ids=[f"{fr.case_id(c)}-{m}" for c, m in MUTANT_CASES])
def test_mutants_are_rejected(data, case, mutant):
    D, H, Hkv, n_seg = case
    q, kc, seg, R = data[case]
    M = fr.reference(q, kc, fr.LENS, seg, n_seg, H, Hkv, D, D ** -0.5, mutate=mutant)
    w = fr.worst(M.flow, R, D)
    print(f"mutant {mutant} {fr.case_id(case)}: err/bound {w:.3g}")
    assert w > 1, "the bound admits the mutant"


def test_one_term_p_is_rejected_on_single_keys_and_rows():
    D, H = 128, 2
    q, kc, seg = fr.single_case(D, H)
    R = fr.reference(q, kc, [32], seg, 32, H, H, D, D ** -0.5)
    assert bool((R.N_ac[0] == torch.ones(32, 32).tril()).all())              # every counted pair is one weight
    two = fr.worst(fr.emulate_f32(q, kc, [32], seg, 32, H, H, D, D ** -0.5), R, D)
    one = fr.worst(fr.emulate_f32(q, kc, [32], seg, 32, H, H, D, D ** -0.5, hi_only=True), R, D)
    print(f"single keys and rows: err/bound hi + lo {two:.3f}, hi only {one:.3f}")
    assert two <= 1 < one


def test_probes_meet_their_conditions():
    for D, H, Hkv, n_seg in ((64, 3, 3, 2), (128, 4, 2, 32)):
        lens = list(fr.LENS)
        seg = fr.make_seg(lens, n_seg)
        q, kc = fr.count_probe(lens, H, Hkv, D)
        R = fr.reference(q, kc, lens, seg, n_seg, H, Hkv, D, D ** -0.5)
        want, ign = fr.count_flow(lens, seg, n_seg)
        assert float((R.flow - want[:, None]).abs().max()) < 1e-11
        assert float((want.sum(-1) + ign - R.rows.double()).abs().max()) < 1e-11 and float(ign.max()) > 0
        q, kc = fr.peak_probe(lens, H, Hkv, D, seg, n_seg)
        assert fr.reference(q, kc, lens, seg, n_seg, H, Hkv, D, D ** -0.5).pmax_min >= fr.W_EXACT


# ------------------------------------------------------------------------------------------------------------------
# the entry point: declared, exported, and its argument checks (host pointers: every refusal comes before any launch)
# ------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_and_refuses_bad_arguments():
    import icl_speech_text_llm_amd.runtime.binding as b
    header = open(os.path.join(ROOT, "include", "icl_hip.h")).read()
    assert re.search(r"^int\s+icl_attn_segflow_bf16\s*\(", header, flags=re.M)
    assert "icl_attn_segflow_bf16" in b.EXPORTED_SYMBOLS and b.ABI_VERSION == 6 and callable(b.attn_segflow)
    lib = b.load_library()
    assert lib.icl_abi_version() == 6
    buf = ctypes.create_string_buffer(4096)                 # 16-byte aligned host memory stands in for every operand
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    good = dict(Q=p, ldq=512, cu=p, Kc=p, seg=p, ld_seg=64, n_seg=4, flow=p, n_seqs=1, n_heads=4, n_kv_heads=0, head_dim=128,
                max_len=64, max_seqlen=64, scale=0.1, stream=None)

    def refused(word, **kw):
        rc = lib.icl_attn_segflow_bf16(*dict(good, **kw).values())
        msg = lib.icl_last_error()
        assert rc == -1 and b"icl_attn_segflow_bf16" in msg and word in msg, (kw, rc, msg)

    for name in ("Q", "cu", "Kc", "seg", "flow"):
        refused(name.encode(), **{name: None})
    refused(b"n_seg", n_seg=0)
    refused(b"n_seg", n_seg=33)
    refused(b"head_dim", head_dim=96)
    refused(b"n_kv_heads", n_kv_heads=3)                                # 4 % 3
    refused(b"n_kv_heads", n_heads=18, n_kv_heads=2, ldq=18 * 128)      # G = 9
    refused(b"head_dim", n_heads=4, n_kv_heads=2, head_dim=64)          # G = 2 at head_dim 64
    refused(b"n_seqs", n_seqs=0)
    refused(b"n_seqs", n_seqs=65536)
    refused(b"max_seqlen", max_seqlen=0)
    refused(b"max_seqlen", max_seqlen=65)
    refused(b"ld_seg", ld_seg=63)
    refused(b"ldq", ldq=516)
    refused(b"ldq", ldq=504)
    refused(b"Q", Q=p + 8)
    refused(b"Kc", Kc=p + 8)
    refused(b"flow", flow=p + 2)
    for bad in (math.inf, -math.inf, math.nan):
        refused(b"scale", scale=bad)
    with pytest.raises(b.IclError, match="no CPU fallback|GPU"):          # the binding takes device operands only
        b.attn_segflow(torch.zeros(1, 512, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int32), torch.zeros(1, 4, 64, 128, dtype=torch.bfloat16),
                       torch.zeros(1, 64, dtype=torch.uint8), torch.zeros(1, 4, 4, 4), 4, 128, 64, 1, 0.1)


def test_runtime_refusals_are_value_errors():
    """``check_readout``'s: FP8 KV, wrong lengths, ids outside 0..255, more than 32 segments."""
    from icl_speech_text_llm_amd.runtime import probes as P
    with pytest.raises(ValueError, match="bf16 KV cache"):
        P.check_readout([[0, 1]], None, "fp8", [2])
    with pytest.raises(ValueError, match="positions"):
        P.check_readout([[0, 1, 1]], None, "bf16", [2])
    with pytest.raises(ValueError, match="0..255"):
        P.check_readout([[0, 256]], None, "bf16", [2])
    with pytest.raises(ValueError, match="at most 32"):
        P.check_readout([list(range(33))], None, "bf16", [33])
    segs, n_seg = P.check_readout([[0, 2, 255]], None, "bf16", [3])
    assert n_seg == 3


# ------------------------------------------------------------------------------------------------------------------
# the runtime: traces, slicing
# ------------------------------------------------------------------------------------------------------------------
def _trace(cname, attrs, kw):
    rec = lt.Recorder()
    rt = lt.generate_runtime(cname, "bf16", rec)
    for k, v in attrs.items():
        setattr(rt, k, v)
    with lt.generate_recording(rec):
        res = rt.prompt_attention(lt.prompts_of(), None, lt.segments_of(lt.GEN_LENS), **kw)
    rec.log.append(lt._result_line(res))
    return rec.text(), res


@pytest.mark.parametrize("cname", ["tiny_h4", "7b_lora", "7b_gqa8_bias"])
@pytest.mark.parametrize("attrs", [{}, dict(prefill_chunk=2)], ids=["one-chunk", "chunk2"])
def test_want_flow_false_is_todays_trace_and_true_adds_one_launch_per_layer(cname, attrs):
    name = "prompt_attention" + ("_chunk2" if attrs else "")
    today = lt.run_prompt_attention(cname, "bf16", name)
    off, res_off = _trace(cname, attrs, dict(want_flow=False))
    assert off == today and res_off.flow is None and res_off.rows is None
    assert "segflow" not in today and "pa_flow" not in today
    on, res_on = _trace(cname, attrs, dict(want_flow=True))
    cfg = lt.configs()[cname]
    n_chunks = -(-len(lt.GEN_LENS) // 2) if attrs else 1
    assert on.count("attn_segflow") == cfg.n_layers * n_chunks and on.count("attn_segmass") == today.count("attn_segmass")
    assert "pa_flow" in on
    n_seg = res_on.mass.shape[-1]
    assert tuple(res_on.flow.shape) == (len(lt.GEN_LENS), cfg.n_layers, cfg.n_heads, n_seg, n_seg)
    assert tuple(res_on.rows.shape) == (len(lt.GEN_LENS), n_seg) and res_on.rows.dtype == torch.int64
    assert ("pfl_q" in today) == (cname == "7b_lora") and "pfl_q" not in on     # the trimmed last layer: in today's 7B trace only


def test_readout_rows_slices_flow():
    from icl_speech_text_llm_amd.runtime import probes as P
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.engines import Workspace
    cfg = SalmonnCfg.tiny().llama
    segs = [torch.tensor(s) for s in ([0, 1, 1], [0, 0, 255, 2], [1], [2, 2])]
    lens = [len(s) for s in segs]
    ws = Workspace("cpu")
    ro = P.readout_state(ws, cfg, segs, 3, lens, 8, False, "cpu", want_flow=True)
    assert tuple(ro.flow.shape) == (cfg.n_layers, 4, cfg.n_heads, 3, 3) and ro.flow.dtype == torch.float32 and ro.probs is None
    assert P.Probes(readout=ro).reads_every_row
    plain = P.readout_state(ws, cfg, segs, 3, lens, 8, False, "cpu")
    assert plain.flow is None and not P.Probes(readout=plain).reads_every_row and not P.Probes().reads_every_row
    ro.flow.copy_(torch.arange(ro.flow.numel(), dtype=torch.float32).view_as(ro.flow))
    part = ro.rows(1, 3)
    assert part.flow.data_ptr() == ro.flow[:, 1:3].data_ptr() and torch.equal(part.flow, ro.flow[:, 1:3])
    assert torch.equal(part.seg, ro.seg[1:3]) and torch.equal(part.mass, ro.mass[:, 1:3]) and part.cu is None
    assert part.flow[0].is_contiguous()                       # what one layer's launch of the chunk writes
    part.start_prefill(lens[1:3], [0, 4, 5])
    assert part.cu.tolist() == [0, 4, 5] and part.max_seqlen == 4 and ro.cu is None
    sub = P.Probes(readout=ro).rows(0, 2)
    assert sub.reads_every_row and tuple(sub.readout.flow.shape) == (cfg.n_layers, 2, cfg.n_heads, 3, 3)

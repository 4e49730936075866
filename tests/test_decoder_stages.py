"""The stage check of the LLM decoder chain (tests/decoder_stage_check.py) without a GPU: LlamaHIP.embed / prefill /
_last_layer_rows / decode_step / logits run on CPU tensors with every runtime.binding wrapper they call replaced by its emulation
(tests/decoder_emulation.py), which reads and writes through the launch's own leading dimensions, offsets, counts, ``pos`` /
``sid`` / ``lens`` and cache addressing.  The host code that chooses the buffers, the offsets, the cache planes, the ``ready``
flag and the gammas is what is under test here: each launch's output must meet the float64 specification of its stage
(oracle/decoder_stages.py), which knows nothing of the launch's arguments.

Every tiny case of tests/test_gpu_decoder_stages.py runs here, one runtime and one workspace per family, in an order that makes
stale contents matter: the largest decode batch first, then the prefill forms, then the smaller batches; an FP8 cache after a
bf16 one.

Second half: twenty planted mistakes.  Each alters the arguments of ONE launch as mistaken host code would have passed them (all
stay inside their buffers) and must be rejected with ``StageFailure`` at the stage it is planted in — which shows that the inputs
(ragged lengths, jittered gains, distinct rows) make each mistake exceed its stage's bound."""
import pytest
import torch

import decoder_emulation as emu
import decoder_stage_check as sc
from oracle import decoder_stages as ds

FAMILIES = ("a", "b", "c", "d", "e", "e_gqa", "f")
A_BATCHES = (65, 64, 9, 8, 1)                 # the LoRA kernel switch (64) and the fp8-weight / fused-RoPE threshold (8)


@pytest.fixture(scope="module", autouse=True)
def emulated():
    with emu.installed():
        yield


_ENV = {}


def _env(name, weight_dtype="bf16", **switches):
    """(cfg, prefix, state dict, state dict the walk reads, runtime, workspace) of one family; made once per module."""
    from icl_speech_text_llm_amd.runtime import engines as E
    key = (name, weight_dtype, tuple(sorted(switches.items())))
    if key not in _ENV:
        cfg, prefix = sc.family_cfg(name)
        sd = sc.family_state(cfg, prefix, "cpu")
        rt = sc.cpu_llama(cfg, sd, prefix, weight_dtype, **switches)
        ds.check_packed_llama(sd, rt, prefix)
        walk_sd = ds.w_prime_state(sd, cfg, prefix) if weight_dtype == "fp8" else sd
        _ENV[key] = (cfg, prefix, sd, walk_sd, rt, E.Workspace("cpu"))
    return _ENV[key]


def _decode(env, Bn, tag, **kw):
    cfg, prefix, sd, walk_sd, rt, ws = env
    worst, counts = sc.run_decode(rt, ws, sd, prefix, Bn, sd_walk=walk_sd, **kw)
    sc.report(f"cpu {tag} decode {Bn}", worst)
    assert max(worst.values()) <= 1.0
    return counts


def _prefill(env, tag, lens=None, **kw):
    cfg, prefix, sd, walk_sd, rt, ws = env
    worst, count, form, _ = sc.run_prefill(rt, ws, walk_sd, prefix, lens or sc.PREFILL_LENS, **kw)
    sc.report(f"cpu {tag} prefill", worst)
    assert max(worst.values()) <= 1.0
    return count, form


def decode_launches(cfg, Bn, fuse_rope=True, fuse_norms=True):
    """Launches of one decode step of a 2-layer decoder: the embedding, per layer [input norm] [LoRA down] QKV, one or two
    launches of RoPE + attention, o (+ norm), gate/up, down (+ norm), then [final norm] LM head."""
    two = not (fuse_rope and Bn > 8 and not cfg.qk_norm and cfg.group == 1)
    per = 1 + (1 if cfg.lora_rank else 0) + 1 + (2 if two else 1) + (3 if fuse_norms else 4)
    return 1 + 2 * per - (1 if fuse_norms else 0) + (1 if fuse_norms else 2)


@pytest.mark.parametrize("name", FAMILIES)
def test_family_prefill_and_decode(name):
    env = _env(name)
    cfg, rt = env[0], env[4]
    lora = 1 if cfg.lora_rank else 0
    full = 1 + 2 * (8 + lora) + 2               # embed, two layers of norm [LoRA] QKV RoPE attention o norm gate/up down, logits
    trims = name in ("a", "b", "f")             # head_dim 128, multi-head, no q/k norm: the trimmed last layer
    assert _decode(env, 65, name) == [decode_launches(cfg, 65)] * 3
    count, form = _prefill(env, name + " last rows", kv="bf16", last_rows_only=True, speech_rows=10 if name == "a" else 0)
    assert form["trim"] == trims and not form["epilogue"] and count == (full + 2 if trims else full + 1)
    rt.prefill_last_rows = False
    try:
        count, form = _prefill(env, name + " untrimmed", kv="bf16", last_rows_only=True)
        assert not form["trim"] and count == full + 1
    finally:
        del rt.prefill_last_rows
    assert _prefill(env, name + " full height", kv="bf16")[0] == full
    assert _prefill(env, name + " no cache")[0] == full
    if name in ("a", "c"):
        assert _prefill(env, name + " fp8 cache", kv="fp8")[0] == full + 2        # + one kv_append_fp8 per layer
    count, form = _prefill(env, name + " two chunks", kv="bf16", chunk=2)
    assert count == 2 * (full - 3 + (2 if trims else 1))                          # no embed, no logits in the chunks' recordings
    for Bn in (A_BATCHES[1:] if name == "a" else (9, 1)):
        assert _decode(env, Bn, name) == [decode_launches(cfg, Bn)] * 3


@pytest.mark.parametrize("weights,kv", [("fp8", "bf16"), ("bf16", "fp8"), ("fp8", "fp8")])
def test_a_fp8_modes(weights, kv):
    """FP8 weights (the walk reads W', which check_packed_llama has shown to be the FP8 rounding of W), an FP8 KV cache in the
    workspace that held the bf16 one, and both."""
    env = _env("a", weights)
    if kv == "fp8":
        _decode(env, 9, f"a w={weights} kv=bf16 first")
    for Bn in A_BATCHES:
        assert _decode(env, Bn, f"a w={weights} kv={kv}", kv=kv) == [decode_launches(env[0], Bn)] * 3
    if weights == "fp8":
        assert env[4].decode_plan(8).sites["qkv"].tile == "fp8w" and env[4].decode_plan(9).sites["qkv"].tile != "fp8w"


@pytest.mark.parametrize("switch", ["fuse_decode_rope", "fuse_decode_norms", "decode_packed_weights"])
def test_a_switches(switch):
    env = _env("a", **{switch: False})
    for Bn in A_BATCHES:
        want = decode_launches(env[0], Bn, fuse_rope=switch != "fuse_decode_rope", fuse_norms=switch != "fuse_decode_norms")
        assert _decode(env, Bn, f"a {switch}=False") == [want] * 3


def test_chain_change_is_named():
    cfg, prefix, sd, _, rt, ws = _env("a")
    with sc.recording() as launches:
        rt.logits(ws, torch.zeros(2, cfg.hidden), xn_ready=True)
    with pytest.raises(sc.ChainChanged, match="update the stage list"):
        sc.Walk(launches, ["rmsnorm", "gemm"])


# ---------------------------------------------------------------------------------------------------------------------------
# planted mistakes: (how the case runs, wrapper, ordinal of that wrapper's launch in the recorded call, edit(arguments, cache,
# runtime), stage that must reject it).  Launch ordinals of family (a), two layers: prefill gemm 0 LoRA down, 1 QKV, 2 o, 3
# gate/up, 4 down, 5 LoRA down of layer 1, then (trimmed) 6 k | v, 7 q; decode at 9 rows gemm_rmsnorm 0 o, 1 down of layer 0, 2 o,
# 3 down of layer 1.
# ---------------------------------------------------------------------------------------------------------------------------
def _plus1(key, row):
    def edit(a, cache, rt):
        t = a[key].clone()
        t[row] += 1
        a[key] = t
    return edit


def _pos_plus1(a, cache, rt):
    _plus1("pos", 2)(a, cache, rt)


def _sid_swapped(a, cache, rt):
    t = a["seq_ids"].clone()
    t[1], t[2] = a["seq_ids"][2], a["seq_ids"][1]
    a["seq_ids"] = t


def _lens_short(a, cache, rt):
    t = a["lens"].clone()
    t[3] -= 1
    a["lens"] = t


def _offsets_swapped(a, cache, rt):
    a["k_off"], a["v_off"] = a["v_off"], a["k_off"]


def _previous_plane(a, cache, rt):
    a["kcache"], a["vcache"] = cache.k[0], cache.v[0]


def _max_len_minus1(a, cache, rt):
    a["max_len"] -= 1


def _lora_block_right(a, cache, rt):
    o = a["out"]
    a["out"] = torch.as_strided(o, o.shape, o.stride(), o.storage_offset() + rt.w.cfg.lora_rank)


def _skip(a, cache, rt):
    return "skip"


def _this_layers_gamma(a, cache, rt):
    a["gamma"] = rt.w.layers[0].rms1


def _rms1_for_final(a, cache, rt):
    a["gamma"] = rt.w.layers[1].rms1


def _no_residual(a, cache, rt):
    a["residual"] = None


def _no_bias(a, cache, rt):
    a["bias"] = None


def _last_idx_next(a, cache, rt):
    _plus1("idx", 1)(a, cache, rt)


def _q_at_s(a, cache, rt):
    r = list(a["rope"])
    r[4] = r[4] + 1
    a["rope"] = tuple(r)


def _whole_cache(a, cache, rt):
    a["kcache"], a["vcache"] = cache.k[0], cache.v[0]


def _v_scales_to_k(a, cache, rt):
    a["vs"] = a["ks"]


def _mha_heads(a, cache, rt):
    a["n_kv_heads"] = a["n_heads"]


def _scale_of_64(a, cache, rt):
    a["scale"] = 64 ** -0.5


def _no_cu_q(a, cache, rt):
    a["cu_q"] = None


D9 = dict(run="decode", Bn=9)
MUTANTS = {
    "01_pos_plus1":          (D9, "attn_decode_rope", 0, _pos_plus1, "L0.rope_q"),
    "02_sid_swapped":        (D9, "attn_decode_rope", 0, _sid_swapped, "L0.cache_k"),
    "03_lens_short":         (D9, "attn_decode_rope", 0, _lens_short, "L0.attn"),
    "04_append_offsets":     (dict(run="prefill", kv="fp8"), "kv_append_fp8", 0, _offsets_swapped, "L0.cache_k"),
    "05_previous_plane":     (D9, "attn_decode_rope", 1, _previous_plane, "L1.cache_k"),
    "06_max_len":            (D9, "attn_decode_rope", 0, _max_len_minus1, "L0.cache_k"),
    "07_lora_block_right":   (dict(run="prefill", kv="bf16"), "gemm", 0, _lora_block_right, "L0.lora_down"),
    "08_lora_skipped":       (dict(run="prefill", kv="bf16"), "gemm", 0, _skip, "L0.lora_down"),
    "09_input_norm_skipped": (D9, "rmsnorm", 0, _skip, "L0.input_norm"),
    "10_this_layers_gamma":  (D9, "gemm_rmsnorm", 1, _this_layers_gamma, "L0.next_norm"),
    "11_rms1_for_final":     (D9, "gemm_rmsnorm", 3, _rms1_for_final, "L1.next_norm"),
    "12_no_residual":        (dict(run="prefill", kv="bf16"), "gemm", 2, _no_residual, "L0.o_proj"),
    "13_no_qkv_bias":        (dict(run="prefill", kv="bf16", family="b"), "gemm", 1, _no_bias, "L0.qkv"),
    "14_last_idx_next":      (dict(run="prefill", kv="bf16", last_rows_only=True), "gather_rows", 0, _last_idx_next, "L1.gather_h"),
    "15_q_rotated_at_s":     (dict(run="prefill", kv="bf16", last_rows_only=True), "gemm", 7, _q_at_s, "L1.q.rope_q"),
    "16_chunk_whole_cache":  (dict(run="prefill", kv="bf16", chunk=2, second=True), "rope_kv", 0, _whole_cache, "L0.cache_k"),
    "17_v_scales_to_k":      (dict(run="decode", Bn=9, kv="fp8"), "attn_decode_rope_fp8", 0, _v_scales_to_k, "L0.cache_k_scale"),
    "18_gqa_as_mha":         (dict(run="decode", Bn=9, family="d"), "attn_decode_gqa", 0, _mha_heads, "L0.attn"),
    "19_scale_of_64":        (dict(run="prefill", kv="bf16"), "attn_fwd", 0, _scale_of_64, "L0.attn"),
    "20_no_cu_q":            (dict(run="prefill", kv="bf16", last_rows_only=True, lens=[1, 5, 3], roomy=True), "attn_fwd", 1, _no_cu_q,
                              "L1.attn"),
}


def _run_mutant(how, mutate):
    """The case a mistake is planted in, on a workspace of its own (a mistake may leave a buffer in a state no clean run does)."""
    from icl_speech_text_llm_amd.runtime import engines as E
    how = dict(how)
    cfg, prefix, sd, _, rt, _ = _env(how.pop("family", "a"))
    ws = E.Workspace("cpu")
    how.pop("second", None)
    if how.pop("roomy", False):          # an earlier, larger batch has left the gathered-row buffers with room for every packed row
        for name, width in (("pfl_q", cfg.hidden), ("pfl_att", cfg.hidden)):
            ws.get(name, (64, width), torch.bfloat16)
    plant = None if mutate is None else (lambda n, k, a, cache: mutate(n, k, a, cache, rt))
    if how.pop("run") == "decode":
        return sc.run_decode(rt, ws, sd, prefix, how.pop("Bn"), mutate=plant, **how)[0]
    return sc.run_prefill(rt, ws, sd, prefix, how.pop("lens", sc.PREFILL_LENS), mutate=plant, **how)[0]


@pytest.mark.parametrize("name", sorted({repr(sorted(m[0].items())): k for k, m in MUTANTS.items()}.values()))
def test_mutant_case_passes_unaltered(name):
    """The inputs of the planted mistakes, unaltered: every stage inside its bound."""
    assert max(_run_mutant(MUTANTS[name][0], None).values()) <= 1.0


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_planted_mistake_is_rejected_at_its_stage(name):
    how, wrapper, ordinal, edit, stage = MUTANTS[name]
    hit, seen = [], []

    def mutate(n, k, arguments, cache, rt):
        if n == wrapper and k == ordinal:
            seen.append(1)
            if how.get("second") and len(seen) < 2:          # the second chunk's launch
                return None
            if not hit:
                hit.append(1)
                return edit(arguments, cache, rt)

    with pytest.raises(sc.StageFailure) as info:
        _run_mutant(how, mutate)
    assert hit == [1], "the launch the mistake is planted in did not happen"
    assert info.value.stage == stage, f"rejected at {info.value.stage}, planted at {stage}: {info.value}"
    print(f"{name}: {info.value}")

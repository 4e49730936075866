"""`-m gpu`: the last decoder layer of a prefill runs only on the rows generation reads (LlamaHIP.prefill(last_rows_only=True),
DESIGN.md §4.4).  Everything here is BIT equality (torch.equal) — the trimmed layer is exact, not approximate: the suffix-query
attention against the full launch's rows, the trimmed prefill against the gather of the full prefill (hidden rows and every
K / V cache plane), and generation with the switch on against generation with it off.

Miniature Llama dims with head_dim 128 (hidden 256, 2 heads, LoRA present), so the trimmed layer's launches are the ones the
7B model takes: the 256x256 tile with the fused RoPE epilogue, the gathers at the augmented K width, the D = 128 causal
attention.  The ragged lengths straddle the 32-row wave block, the 64-key tile and the 128-row q-block."""
import os

import pytest
import torch

from decoder_support import row_prompts
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
LENS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 376]
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EOS, PAD = 2, 400


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def _rand_bf16(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(DEV)


# ---- 1. the suffix-query attention ------------------------------------------------------------------------------------------------
H_ATT, D_ATT, MAXLEN_ATT = 3, 128, 384


@pytest.fixture(scope="module")
def attn_case(B):
    """q / k / v of the ragged batch and the FULL causal launch's output: the one reference of the attention tests."""
    M = sum(LENS)
    q, k, v = (_rand_bf16(M, H_ATT * D_ATT, seed=811 + i) for i in range(3))
    cu = torch.tensor(_cu(LENS), dtype=torch.int32, device=DEV)
    full = torch.empty(M, H_ATT * D_ATT, dtype=torch.bfloat16, device=DEV)
    B.attn_fwd(q, k, v, full, cu, max(LENS), H_ATT, D_ATT, D_ATT ** -0.5, causal=True)
    torch.cuda.synchronize()
    return q, k, v, cu, full


@pytest.mark.parametrize("kv", ["packed", "cache"])
@pytest.mark.parametrize("q_len", [1, 33])
def test_suffix_attention_matches_the_full_launch_bitwise(B, attn_case, q_len, kv):
    """Each sequence attends with its last min(q_len, len) queries only, packed by their own offsets: every output row equals the
    full launch's row at the same position, bit for bit — with K / V packed next to where Q came from and with K / V in the cache
    layout (rows past a sequence's length hold NaN and must never reach the output)."""
    q, k, v, cu, full = attn_case
    cu_h = _cu(LENS)
    qlens = [min(q_len, n) for n in LENS]
    rows = torch.tensor([cu_h[s + 1] - ql + i for s, ql in enumerate(qlens) for i in range(ql)], device=DEV)
    cu_q = torch.tensor(_cu(qlens), dtype=torch.int32, device=DEV)
    q_sfx = q[rows].contiguous()
    out = torch.full((len(rows) + 2, H_ATT * D_ATT), 7.0, dtype=torch.bfloat16, device=DEV)      # 2 guard rows below
    if kv == "packed":
        B.attn_fwd(q_sfx, k, v, out, cu, max(LENS), H_ATT, D_ATT, D_ATT ** -0.5, causal=True, cu_q=cu_q)
    else:
        kc = torch.full((len(LENS), H_ATT, MAXLEN_ATT, D_ATT), float("nan"), dtype=torch.bfloat16, device=DEV)
        vc = torch.full_like(kc, float("nan"))
        for s, n in enumerate(LENS):
            kc[s, :, :n] = k[cu_h[s]:cu_h[s + 1]].view(n, H_ATT, D_ATT).transpose(0, 1)
            vc[s, :, :n] = v[cu_h[s]:cu_h[s + 1]].view(n, H_ATT, D_ATT).transpose(0, 1)
        B.attn_fwd(q_sfx, kc, vc, out, cu, max(LENS), H_ATT, D_ATT, D_ATT ** -0.5, causal=True, kv_cache_max_len=MAXLEN_ATT,
                   cu_q=cu_q)
    torch.cuda.synchronize()
    assert torch.equal(out[:len(rows)], full[rows])
    assert bool((out[len(rows):] == 7.0).all())


def test_suffix_attention_rejects_what_it_is_not_built_for(B, attn_case):
    q, k, v, cu, full = attn_case
    cu_q = torch.arange(len(LENS) + 1, dtype=torch.int32, device=DEV)
    out = torch.empty(len(LENS), H_ATT * D_ATT, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="suffix-query form"):
        B.attn_fwd(q[:len(LENS)], k, v, out, cu, max(LENS), H_ATT, D_ATT, D_ATT ** -0.5, causal=False, cu_q=cu_q)


def test_gather_rows_bf16(B):
    src = _rand_bf16(50, 320, seed=5)
    idx = torch.tensor([49, 0, 7, 7, 31], dtype=torch.int32, device=DEV)
    out = torch.empty(5, 320, dtype=torch.bfloat16, device=DEV)
    B.gather_rows(src, idx, out)
    assert torch.equal(out, src[idx.long()])


# ---- 2. / 3. the trimmed prefill and generation --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    cfg = SalmonnCfg.tiny(use_beats=False, lora=True, vocab=401)
    sd = synth.salmonn_state(cfg, seed=3, jitter=True, parts=("llama",))
    rt = SalmonnRuntime(cfg, dict(sd), device=DEV, parts=("llama",))
    assert cfg.llama.head_dim == 128 and rt.llama.w.layers[-1].lora_a is not None
    return cfg, rt


def test_trimmed_prefill_matches_the_full_prefill_bitwise(B, env):
    """prefill(last_rows_only=True) == the last rows of the full prefill, and every layer's K and V cache planes are the same
    bits after either (LoRA present: the augmented columns of the gathered rows are covered)."""
    cfg, rt = env
    c, ll, ws = cfg.llama, rt.llama, rt.ws
    assert ll.prefill_last_rows and B.rope_epilogue_ok(c.n_heads, c.head_dim, ll.w.k_aug)
    prompts = row_prompts(cfg.llama.vocab, LENS, seed=4300)
    last_idx = torch.tensor([e - 1 for e in _cu(LENS)[1:]], device=DEV)

    def run(trim):
        h, lens = rt.embed_prompts(prompts, None)
        assert lens == LENS
        cache = rt._cache(len(LENS), 384)
        cache.k.fill_(float("nan"))
        cache.v.fill_(float("nan"))
        if trim:
            last = ll.prefill(ws, h, lens, cache, last_rows_only=True).clone()
        else:
            last = ll.prefill(ws, h, lens, cache)[last_idx].clone()
        torch.cuda.synchronize()
        return last, cache.k.clone(), cache.v.clone()

    full, k_full, v_full = run(False)
    ws.release("pfl_q")
    trimmed, k_trim, v_trim = run(True)
    assert ("pfl_q", torch.bfloat16) in ws._bufs, "the trimmed last layer did not run"
    assert torch.isfinite(full).all()
    assert torch.equal(trimmed, full)
    for i in range(c.n_layers):        # bit patterns: the never-written positions hold the NaN fill in both
        assert torch.equal(k_trim[i].view(torch.int16), k_full[i].view(torch.int16)), f"layer {i}: K cache differs"
        assert torch.equal(v_trim[i].view(torch.int16), v_full[i].view(torch.int16)), f"layer {i}: V cache differs"
    # written where it must be: every position below a sequence's length is finite in the last layer's planes
    for s, n in enumerate(LENS):
        assert torch.isfinite(k_trim[-1, s, :, :n].float()).all() and torch.isfinite(v_trim[-1, s, :, :n].float()).all()


@pytest.fixture(scope="module")
def auto():
    from icl_speech_text_llm_amd.data.task_configs import DatasetType
    from icl_speech_text_llm_amd.runtime.constraints import build_label_automaton
    from icl_speech_text_llm_amd.utils.tokenization import load_llama_tokenizer
    return build_label_automaton(load_llama_tokenizer(os.path.join(G, "llama_spm"), 401), list(DatasetType))


@pytest.mark.parametrize("batch", ["one", "ragged_chunks"])
@pytest.mark.parametrize("mode", ["greedy", "constrained", "beam4"])
def test_generation_is_unchanged_by_the_switch(env, auto, mode, batch):
    """Tokens and first-step logits of generate() with the trimmed last layer == with the full-height one (the switch off), for
    greedy, label-constrained and 4-beam decoding; one prompt, and 11 prompts prefilled in chunks of 4 (a ragged last chunk)."""
    cfg, rt = env
    lens = LENS[-1:] if batch == "one" else LENS
    prompts = row_prompts(cfg.llama.vocab, lens, seed=4400)
    kw = dict(max_new_tokens=4, want_first_logits=True)
    if mode == "greedy":
        kw.update(suppress_eos=True)
    elif mode == "constrained":
        kinds = ["voxceleb", "hvb", "sqa", "voxpopuli"]
        kw.update(eos_id=EOS, pad_id=PAD, max_new_tokens=10, constraint=(auto, [auto.starts[kinds[i % 4]] for i in range(len(lens))]))
    else:
        kw.update(suppress_eos=True, num_beams=4)
    keep_chunk, keep_switch = rt.prefill_chunk, rt.llama.prefill_last_rows
    try:
        rt.prefill_chunk = 4
        out = {}
        for on in (False, True):
            rt.llama.prefill_last_rows = on
            res = rt.generate(prompts, None, **kw)
            out[on] = (res.tokens.clone(), res.first_logits.clone())
    finally:
        rt.prefill_chunk, rt.llama.prefill_last_rows = keep_chunk, keep_switch
    assert torch.isfinite(out[True][1]).all()
    assert torch.equal(out[True][1], out[False][1]), "first-step logits differ"
    assert torch.equal(out[True][0], out[False][0]), "tokens differ"

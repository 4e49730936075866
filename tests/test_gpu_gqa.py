"""`-m gpu`: grouped-query attention (GQA).  The three kernels against the float64 reference and probes of oracle/attention.py
(K / V expanded per group, so the reference is the multi-head one at H = Hkv * G heads), and a GQA decoder (hidden 512, 4 query /
2 K/V heads, head_dim 128) through the runtimes and the plugin against the CPU oracle and against its multi-head twin — the same
model with the k_proj / v_proj rows (biases, lora_B) repeated per group, whose oracle logits are the same tensor.

Measured on MI355X (printed by the tests, recorded in DESIGN.md): decode err / bound 0.48-0.49 on normal data and 0.21-0.23 on offset
data, 100 % of the output elements bit-equal to icl_attn_decode_bf16 on the expanded cache at G = 2, 3, 4, 5, 7 (99.997 % at G = 6,
99.9993 % at G = 8); prefill 0.48-0.49 / 0.23 and torch.equal to the multi-head launch; decoder chain worst step rel-L2 3.14e-3 (4 rows)
and 3.68e-3 (12 rows), the multi-head twin the same to four digits (ratio 1.000); forward logits 2.65e-3 (SALMONN decoder), 2.74e-3
(Qwen2 decoder); FP8 weight mode 3.37e-3 / 3.71e-3 against the oracle on W'."""
from dataclasses import replace

import pytest
import torch

from decoder_support import llama_oracle, row_prompts, teacher_forced_check
from fp8_ref import w_prime_state
from gpu_support import DEV, B, dev, stop_after_a_device_fault  # noqa: F401  (fixtures)
from oracle import attention as oa

pytestmark = pytest.mark.gpu

D = 128
PARITY_RATIO = 1.25       # the project's margin between two runs that differ only in summation order


def _expand(x, Hkv, G):
    """Packed [rows, Hkv * D] -> [rows, Hkv * G * D]: K/V head j becomes heads j * G .. j * G + G - 1."""
    return x.view(x.shape[0], Hkv, D).repeat_interleave(G, dim=1).reshape(x.shape[0], Hkv * G * D)


def _gqa_data(kind, lens, Hkv, G, causal=True):
    """(q [total, H * D], k, v [total, Hkv * D]) on the device: the probes of oracle/attention.py with a K/V head shared by G
    query heads.  peak: build g (head_offset = g) has the same k / v for every g; query head kvh * G + g takes build g's q."""
    H = Hkv * G
    if kind == "count":
        q = torch.zeros(sum(lens), H * D, dtype=torch.bfloat16)
        _, k, v = oa.probe_count(lens, Hkv, D)
    elif kind == "peak":
        builds = [oa.probe_peak(lens, Hkv, D, causal=causal, head_offset=g) for g in range(G)]
        k, v = builds[0][1], builds[0][2]
        assert all(torch.equal(b[1], k) and torch.equal(b[2], v) for b in builds)
        q = torch.stack([b[0].view(-1, Hkv, D) for b in builds], dim=2).reshape(-1, H * D)      # [total, Hkv, G, D]
    else:
        q = oa.random_data(lens, H, D, offset=kind == "offset")[0]
        _, k, v = oa.random_data(lens, Hkv, D, oa.SEED + 1, offset=kind == "offset")
    return dev(q, k, v)


# ------------------------------------------------------------------------------------------------------------------
# 1. icl_attn_decode_gqa_bf16
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hkv,G", [(2, 2), (2, 4), (1, 7), (3, 8), (2, 3), (1, 5), (1, 6)])
def test_decode_gqa(B, Hkv, G):
    """Count, peak and random / offset data over DECODE_LENS (the launcher has no few / many switch: one instantiation per group
    size, all seven run here).  Also prints the share of output elements bit-equal to icl_attn_decode_bf16 on the expanded cache."""
    lens, max_len, scale, H = list(oa.DECODE_LENS), 320, D ** -0.5, Hkv * G
    n, hd = len(lens), H * D
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    name = f"attn_decode_gqa {n}x{Hkv}x{G}"
    same = total = 0

    def run(q, k, v):
        nonlocal same, total
        kc, vc = oa.to_cache(k, v, lens, Hkv, D, max_len)                          # NaN past each length
        kx, vx = oa.to_cache(_expand(k, Hkv, G), _expand(v, Hkv, G), lens, H, D, max_len)
        obuf = torch.full((n, hd + 24), float("nan"), dtype=torch.bfloat16, device=DEV)
        out = obuf[:, 8:8 + hd]
        qbuf = torch.zeros(n, hd + 64, dtype=torch.bfloat16, device=DEV)
        qbuf[:, 32:32 + hd] = oa.last_rows(q, lens)
        B.attn_decode_gqa(qbuf[:, 32:32 + hd], kc, vc, out, lens_t, H, Hkv, D, max_len, scale)
        assert bool(torch.isnan(obuf[:, :8].float()).all()) and bool(torch.isnan(obuf[:, 8 + hd:].float()).all()), f"{name}: wrote outside O"
        mha = torch.empty(n, hd, dtype=torch.bfloat16, device=DEV)
        B.attn_decode(qbuf[:, 32:32 + hd], kx, vx, mha, lens_t, H, D, max_len, scale)
        same += int((out.view(torch.int16) == mha.view(torch.int16)).sum())
        total += out.numel()
        return out.reshape(n, H, D), oa.decode_ref(oa.last_rows(q, lens), kx, vx, lens, H, D, scale)

    out, R = run(*_gqa_data("count", lens, Hkv, G))
    oa.assert_count(out, R, name)
    out, R = run(*_gqa_data("peak", lens, Hkv, G))
    oa.assert_exact(out, R, None, name)
    for data in ("normal", "offset"):
        out, R = run(*_gqa_data(data, lens, Hkv, G))
        print(f"err/bound {name} {data}: {oa.assert_bound(out, R, D, oa.R_P['decode'], f'{name} {data}'):.3f}")
    print(f"{name}: {same}/{total} = {same / total:.4%} of the output elements bit-equal to attn_decode on the expanded cache")


def test_decode_gqa_argument_checks(B):
    q = torch.zeros(2, 4 * D, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(2, 2, 64, D, dtype=torch.bfloat16, device=DEV)
    lens = torch.ones(2, dtype=torch.int32, device=DEV)
    out = torch.empty_like(q)
    with pytest.raises(B.IclError):
        B.attn_decode_gqa(q, kc, kc, out, lens, 4, 3, D, 64, 1.0)          # 4 % 3
    with pytest.raises(B.IclError):
        B.attn_decode_gqa(q[:, :256], kc, kc, out, lens, 4, 2, 64, 64, 1.0)  # GQA at head_dim 64
    with pytest.raises(B.IclError):
        B.attn_decode_gqa(q, kc, kc, out, lens, 16, 1, D, 64, 1.0)         # 16 query heads per K/V head


# ------------------------------------------------------------------------------------------------------------------
# 2. prefill: icl_attn_fwd_bf16 / icl_attn_fwd_suffix_bf16 with n_kv_heads
# ------------------------------------------------------------------------------------------------------------------
def _fwd(B, q, k, v, lens, H, Hkv, *, cache=False, **kw):
    out = torch.full((sum(lens), H * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    cu = torch.tensor(oa.cu_of(lens), dtype=torch.int32, device=DEV)
    if cache:
        k, v = oa.to_cache(k, v, lens, Hkv, D, max(lens))
        kw["kv_cache_max_len"] = max(lens)
    B.attn_fwd(q, k, v, out, cu, max(lens), H, D, D ** -0.5, causal=True, n_kv_heads=0 if Hkv == H else Hkv, **kw)
    return out.view(-1, H, D)


@pytest.mark.parametrize("Hkv,G", [(1, 2), (2, 4), (1, 7)])
def test_prefill_gqa(B, Hkv, G):
    lens, H, scale = list(oa.PREFILL_LENS), Hkv * G, D ** -0.5
    cu = oa.cu_of(lens)
    name = f"attn_fwd gqa {Hkv}x{G}"
    last = torch.tensor([c - 1 for c, L in zip(cu[1:], lens) if L], device=DEV)
    cu_q = torch.tensor(oa.cu_of([min(L, 1) for L in lens]), dtype=torch.int32, device=DEV)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    for kind in ("count", "peak", "normal", "offset"):
        q, k, v = _gqa_data(kind, lens, Hkv, G)
        kx, vx = _expand(k, Hkv, G), _expand(v, Hkv, G)
        R = oa.prefill_ref(q, kx, vx, lens, H, D, scale, causal=True)
        want = _fwd(B, q, kx, vx, lens, H, H)                                # the multi-head launch on the expanded K / V
        for cache in (False, True):
            out = _fwd(B, q, k, v, lens, H, Hkv, cache=cache)
            what = f"{name} {kind} cache={int(cache)}"
            if kind == "count":
                oa.assert_count(out, R, what)
            elif kind == "peak":
                oa.assert_exact(out, R, None, what)
            else:
                print(f"err/bound {what}: {oa.assert_bound(out, R, D, oa.R_P['prefill128'], what):.3f}")
            assert torch.equal(out, want), f"{what}: differs from the n_kv_heads = 0 launch on the expanded K / V"
            # the suffix form, q_len = 1: the last row of every sequence, bit for bit
            sfx = torch.full((int(cu_q[-1]), H * D), float("nan"), dtype=torch.bfloat16, device=DEV)
            kk, vv = (oa.to_cache(k, v, lens, Hkv, D, max(lens)) if cache else (k, v))
            B.attn_fwd(q[last].contiguous(), kk, vv, sfx, cu_t, max(lens), H, D, scale, causal=True, cu_q=cu_q, n_kv_heads=Hkv,
                       kv_cache_max_len=max(lens) if cache else 0)
            assert torch.equal(sfx.view(-1, H, D), want[last]), f"{what}: suffix form != the full launch's last rows"


def test_prefill_gqa_argument_checks(B):
    q = torch.zeros(4, 4 * 64, dtype=torch.bfloat16, device=DEV)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    with pytest.raises(B.IclError):
        B.attn_fwd(q, q, q, torch.empty_like(q), cu, 4, 4, 64, 0.125, causal=True, n_kv_heads=2)     # GQA at head_dim 64
    q = torch.zeros(4, 4 * D, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(B.IclError):
        B.attn_fwd(q, q, q, torch.empty_like(q), cu, 4, 4, D, 0.1, causal=True, n_kv_heads=3)        # 4 % 3


# ------------------------------------------------------------------------------------------------------------------
# 3. icl_rope_kv_gqa_bf16
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hkv", [(4, 2), (7, 1), (4, 4)])
def test_rope_kv_gqa(B, H, Hkv):
    """q block, k block and the appended cache rows against icl_rope_kv_bf16 on the buffer with k / v expanded to H heads (K/V
    head j <-> expanded head j * G); rows never addressed keep their NaN; n_kv_heads == n_heads is the old entry point."""
    M, n_seqs, max_len, G = 37, 5, 48, H // Hkv
    g = torch.Generator().manual_seed(11)
    pos = torch.randint(1, max_len - 1, (M,), generator=g)
    pos[0], pos[1] = 0, max_len - 1
    sid = torch.arange(M) % n_seqs
    # distinct (sequence, position) pairs, sequences in a permuted order
    taken = set()
    for m in range(M):
        while (int(sid[m]), int(pos[m])) in taken:
            pos[m] = (int(pos[m]) + 1) % max_len
        taken.add((int(sid[m]), int(pos[m])))
    perm = torch.randperm(M, generator=g)
    pos, sid = pos[perm].to(torch.int32).to(DEV), sid[perm].to(torch.int32).to(DEV)
    assert 0 in pos.tolist() and max_len - 1 in pos.tolist()
    half = D // 2
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    ang = torch.arange(max_len, dtype=torch.float32)[:, None] * inv[None]
    cos, sin = ang.cos().to(DEV), ang.sin().to(DEV)
    q = torch.randn(M, H * D, generator=g).to(torch.bfloat16)
    k = torch.randn(M, Hkv * D, generator=g).to(torch.bfloat16)
    v = torch.randn(M, Hkv * D, generator=g).to(torch.bfloat16)
    pad = torch.zeros(M, 16, dtype=torch.bfloat16)
    k_off, v_off = H * D + 16, H * D + 16 + Hkv * D
    buf = torch.cat([q, pad, k, v, pad], 1).to(DEV)
    kc = torch.full((n_seqs, Hkv, max_len, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    vc = torch.full_like(kc, float("nan"))
    B.rope_kv_gqa(buf, k_off, v_off, cos, sin, pos, sid, kc, vc, H, Hkv, D, max_len)
    # the multi-head call on the expanded buffer
    xk_off, xv_off = H * D + 16, 2 * H * D + 16
    xbuf = torch.cat([q, pad, _expand(k, Hkv, G), _expand(v, Hkv, G), pad], 1).to(DEV)
    xkc = torch.full((n_seqs, H, max_len, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    xvc = torch.full_like(xkc, float("nan"))
    B.rope_kv(xbuf, xk_off, xv_off, cos, sin, pos, sid, xkc, xvc, H, D, max_len)
    bits = lambda t: t.contiguous().view(torch.int16)
    assert torch.equal(bits(buf[:, :H * D]), bits(xbuf[:, :H * D])), "q block"
    xk = xbuf[:, xk_off:xk_off + H * D].view(M, Hkv, G, D)[:, :, 0].reshape(M, Hkv * D)
    assert torch.equal(bits(buf[:, k_off:k_off + Hkv * D]), bits(xk)), "k block"
    assert torch.equal(bits(buf[:, v_off:v_off + Hkv * D]), bits(v.to(DEV))), "v block is left alone"
    assert torch.equal(bits(buf[:, H * D:k_off]), bits(pad.to(DEV))) and torch.equal(bits(buf[:, v_off + Hkv * D:]), bits(pad.to(DEV)))
    assert torch.equal(bits(kc), bits(xkc[:, ::G])) and torch.equal(bits(vc), bits(xvc[:, ::G])), "cache rows (NaN where not addressed)"
    written = torch.zeros(n_seqs, max_len, dtype=torch.bool, device=DEV)
    written[sid.long(), pos.long()] = True
    assert int(written.sum()) == M
    for c in (kc, vc):
        nan = torch.isnan(c.float())
        assert bool(nan[~written[:, None].expand(-1, Hkv, -1)].all()) and not bool(nan[written[:, None].expand(-1, Hkv, -1)].any())
    if H == Hkv:
        assert torch.equal(bits(buf), bits(xbuf))


# ------------------------------------------------------------------------------------------------------------------
# 4 - 8. the GQA decoder through the runtimes and the plugin
# ------------------------------------------------------------------------------------------------------------------
def _gqa_llama(base, **kw):
    return replace(base, hidden=512, n_layers=2, n_heads=4, n_kv_heads=2, ffn=1024, **kw)


def _twin_state(sd, c, prefix):
    """The multi-head twin's checkpoint: k_proj / v_proj rows (weights, biases, lora_B) repeated per group."""
    out = dict(sd)
    for key, t in sd.items():
        if key.startswith(prefix + "model.layers.") and (".k_proj." in key or ".v_proj." in key) and ".lora_A." not in key:
            out[key] = t.view(c.kv_heads, c.head_dim, *t.shape[1:]).repeat_interleave(c.group, 0).reshape(c.hidden, *t.shape[1:])
    return out


@pytest.fixture(scope="module")
def gqa_env():
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    tiny = SalmonnCfg.tiny(use_beats=False)
    cfg = replace(tiny, llama=_gqa_llama(tiny.llama))
    assert cfg.llama.lora_targets == ("q_proj", "v_proj") and cfg.llama.lora_rank == 8 and cfg.llama.group == 2
    sd = synth.salmonn_state(cfg, seed=0, jitter=True, parts=("llama",))
    rt = SalmonnRuntime(cfg, dict(sd), device=DEV, parts=("llama",))
    tcfg = replace(cfg, llama=replace(cfg.llama, n_kv_heads=None))
    twin = SalmonnRuntime(tcfg, _twin_state(sd, cfg.llama, "llama_model."), device=DEV, parts=("llama",))
    return cfg, sd, rt, twin


@pytest.mark.parametrize("lens", [[33, 90, 61, 12], [33, 90, 61, 12, 5, 70, 44, 21, 9, 57, 28, 16]], ids=["4rows", "12rows"])
def test_decoder_chain(gqa_env, lens):
    """Prefill + 10 decode steps of the GQA model, teacher-forced against LlamaOracle(n_kv_heads=2); the multi-head twin runs
    today's path against the same oracle logits, and the GQA run's worst step rel-L2 is within PARITY_RATIO of the twin's."""
    cfg, sd, rt, twin = gqa_env
    assert rt.llama.w.layers[0].wqkv.shape == (1024, 576) and twin.llama.w.layers[0].wqkv.shape == (1536, 576)
    prompts = row_prompts(cfg.llama.vocab, lens, seed=7)
    ob = llama_oracle(sd, cfg.llama, "llama_model.")
    e_gqa = teacher_forced_check(rt, ob, prompts, "gqa")
    e_twin = teacher_forced_check(twin, ob, prompts, "twin")
    print(f"decoder chain {len(lens)} rows: worst step rel-L2 gqa {e_gqa:.3e}, multi-head twin {e_twin:.3e}, ratio {e_gqa / e_twin:.3f}")
    assert e_gqa <= PARITY_RATIO * e_twin


def test_forward_logits_and_sampling(gqa_env):
    """Teacher-forced forward (no cache: packed q | k | v rows) against the oracle, and a sampled run (the sampling kernels never
    see heads: it only has to run and repeat under the same generator seed)."""
    cfg, sd, rt, twin = gqa_env
    prompts = row_prompts(cfg.llama.vocab, [37, 150, 64], seed=3)
    ob = llama_oracle(sd, cfg.llama, "llama_model.")
    want = torch.cat([ob.forward(ob.embed(torch.tensor(p[0]))[None])[0][0] for p in prompts])
    rel = lambda a: float((a.float().cpu() - want).norm() / want.norm())
    got, n = rt.forward_logits(prompts, None)
    e_gqa = rel(got.clone())
    e_twin = rel(twin.forward_logits(prompts, None)[0])
    print(f"forward logits rel-L2 vs oracle: gqa {e_gqa:.3e}, multi-head twin {e_twin:.3e}")
    assert n == [37, 150, 64] and e_gqa <= PARITY_RATIO * e_twin
    outs = [rt.generate(prompts, None, max_new_tokens=6, do_sample=True, temperature=0.8, top_p=0.9, suppress_eos=True,
                        generator=torch.Generator(device=DEV).manual_seed(5)).tokens for _ in range(2)]
    assert outs[0].shape == (3, 6) and torch.equal(outs[0], outs[1])


def test_margin_weights_greedy_and_beam():
    """Decisive-margin weights: greedy ids are the designed successor chain; num_beams=3 returns the oracle's beam ids."""
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    tiny = SalmonnCfg.tiny(use_beats=False)
    cfg = replace(tiny, llama=_gqa_llama(tiny.llama))
    sd = synth.salmonn_state(cfg, seed=1, parts=("llama",), margin=True)
    rt = SalmonnRuntime(cfg, dict(sd), device=DEV, parts=("llama",))
    for lens in ([33, 90, 61, 12], [20 + 3 * i for i in range(12)]):
        prompts = row_prompts(cfg.llama.vocab, lens, seed=21)
        gen = rt.generate(prompts, None, max_new_tokens=8, suppress_eos=True)
        for b, p in enumerate(prompts):
            chain, t = [], p[0][-1]
            for _ in range(8):
                t = synth.margin_successor(sd, t)
                chain.append(t)
            assert gen.tokens[b].tolist() == chain, (len(lens), b)
    prompts = row_prompts(cfg.llama.vocab, [33, 90, 61], seed=21)
    beams = rt.generate(prompts, None, max_new_tokens=5, suppress_eos=True, num_beams=3)
    ob = llama_oracle(sd, cfg.llama, "llama_model.")
    for b, p in enumerate(prompts):
        want = ob.generate_beam(ob.embed(torch.tensor(p[0]))[None], 5, -1, cfg.llama.pad_id, 3, 1.0)
        assert beams.tokens[b, :want.shape[1]].tolist() == want[0].tolist(), b


def test_fp8_weight_mode_on_the_gqa_model(gqa_env):
    """llm_weight_dtype="fp8" with GQA: generate at 4 rows (the fp8-weight skinny kernel) and 12 rows (the bf16 tiles on W'),
    teacher-forced against the oracle given W' (rebuilt on the CPU with torch.float8_e4m3fn)."""
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    cfg, sd, _, _ = gqa_env
    r8 = SalmonnRuntime(cfg, dict(sd), device=DEV, parts=("llama",), llm_weight_dtype="fp8")
    wsd = w_prime_state(sd, cfg.llama)
    for L, i in zip(r8.llama.w.layers, range(2)):
        want = torch.cat([wsd[f"llama_model.model.layers.{i}.self_attn.{n}_proj.weight"] for n in "qkv"])
        assert torch.equal(L.wqkv[:, :512].float().cpu(), want)
    ob = llama_oracle(wsd, cfg.llama, "llama_model.")
    for lens in ([33, 90, 61, 12], [33, 90, 61, 12, 5, 70, 44, 21, 9, 57, 28, 16]):
        e = teacher_forced_check(r8, ob, row_prompts(cfg.llama.vocab, lens, seed=7), f"fp8w {len(lens)} rows")
        print(f"fp8 weight mode, gqa, {len(lens)} rows: worst step rel-L2 vs the oracle on W' {e:.3e}")


def test_plugin_loads_a_gqa_hf_folder(tmp_path):
    """CustomSALMONN(llama_path=<HF folder whose config.json has num_key_value_heads=2>) loads and generates."""
    from transformers import LlamaConfig, LlamaForCausalLM, WhisperConfig, WhisperModel
    from icl_speech_text_llm_amd.models.custom_salmon import CustomSALMONN
    from icl_speech_text_llm_amd.utils.tokenization import ByteTokenizer
    from oracle import models as om
    torch.manual_seed(0)
    llama = LlamaForCausalLM(LlamaConfig(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                         intermediate_size=1024, vocab_size=259, rms_norm_eps=1e-5, max_position_embeddings=2048,
                                         tie_word_embeddings=False)).eval()
    whisper = WhisperModel(WhisperConfig(d_model=128, encoder_layers=2, encoder_attention_heads=2, encoder_ffn_dim=256,
                                         decoder_layers=1, decoder_attention_heads=2, decoder_ffn_dim=64, num_mel_bins=80,
                                         max_source_positions=1500, vocab_size=64, pad_token_id=0, bos_token_id=1, eos_token_id=2,
                                         decoder_start_token_id=1)).eval()
    with torch.no_grad():
        for p in llama.parameters():
            if p.dim() > 1:
                p.mul_(3.0)                                         # away from the N(0, 0.02) near-degenerate regime
    llama.save_pretrained(tmp_path / "llama", safe_serialization=True)
    whisper.save_pretrained(tmp_path / "whisper", safe_serialization=True)
    m = CustomSALMONN(llama_path=str(tmp_path / "llama"), whisper_path=str(tmp_path / "whisper"), beats_path="", lora=False,
                      ckpt_path="", device=DEV, tokenizer=ByteTokenizer(260)).eval()
    c = m.cfg.llama
    assert (c.hidden, c.n_heads, c.n_kv_heads, c.group, c.head_dim, c.vocab) == (512, 4, 2, 2, 128, 260)
    assert m.salmonn.state_dict()["llama_model.model.layers.0.self_attn.k_proj.weight"].shape == (256, 512)
    prompts = ["classify this sentence please.\nOutput:", "is it positive?\nOutput:", "short\nOutput:"]
    batch = {"prompt": prompts, "num_examples": torch.tensor([0, 0, 0]), "max_new_tokens": 6}
    texts = m.generate_output(dict(batch))
    assert isinstance(texts, list) and len(texts) == 3 and all(isinstance(t, str) for t in texts)
    res = m.generate_ids(dict(batch), want_first_logits=True)
    sd = {k: v.detach().float() for k, v in llama.state_dict().items()}
    ob = om.LlamaOracle(sd, 4, 1e-5, rnd=om.bf16_round, n_kv_heads=2)
    for b, prompt in enumerate(prompts):
        ids = m.llama_tokenizer(prompt, add_special_tokens=False, return_tensors="pt")["input_ids"]
        _, first = ob.generate_greedy(ob.embed(ids[0])[None], 1, -1, 259, return_first_logits=True)
        got, first = res.first_logits[b, :259].float().cpu(), first[0]
        err = float((got - first).abs().max())
        top2 = first.topk(2)
        chosen = int(res.tokens[b, 0])
        print(f"plugin gqa row {b}: first-logit max abs err {err:.2e}, oracle margin {float(top2.values[0] - top2.values[1]):.2e}")
        assert float(top2.values[0] - first[chosen]) <= 2 * err + 1e-6
        if float(top2.values[0] - top2.values[1]) > 4 * err:
            assert chosen == int(top2.indices[0])


def test_qwen_gqa_forward_matches_oracle():
    """QwenAudioCfg.tiny() with a GQA llm (q / k / v biases, LoRA on q and k): forward logits against the oracle within
    PARITY_RATIO of the multi-head twin's distance."""
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import QwenAudioCfg
    from icl_speech_text_llm_amd.runtime.qwen import QwenAudioRuntime
    q = QwenAudioCfg.tiny()
    cfg = replace(q, llm=_gqa_llama(q.llm))
    assert cfg.llm.qkv_bias and cfg.llm.lora_targets == ("q_proj", "k_proj")
    sd = synth.qwen_audio_state(cfg, seed=0)
    assert sd["language_model.model.layers.0.self_attn.k_proj.lora_B.weight"].shape == (256, 8)
    rt = QwenAudioRuntime(cfg, dict(sd), device=DEV)
    twin = QwenAudioRuntime(replace(cfg, llm=replace(cfg.llm, n_kv_heads=None)), _twin_state(sd, cfg.llm, "language_model."), device=DEV)
    prompts = row_prompts(cfg.llm.vocab - 1, [37, 150, 64], seed=9)          # below the audio token id
    ob = llama_oracle(sd, cfg.llm, "language_model.")
    want = torch.cat([ob.forward(ob.embed(torch.tensor(p[0]))[None])[0][0] for p in prompts])
    rel = lambda a: float((a.float().cpu() - want).norm() / want.norm())
    e_gqa = rel(rt.forward_logits(prompts, None)[0])
    e_twin = rel(twin.forward_logits(prompts, None)[0])
    print(f"qwen forward logits rel-L2 vs oracle: gqa {e_gqa:.3e}, multi-head twin {e_twin:.3e}, ratio {e_gqa / e_twin:.3f}")
    assert e_gqa <= PARITY_RATIO * e_twin
    res = rt.generate(prompts, None, max_new_tokens=4, suppress_eos=True)
    assert res.tokens.shape == (3, 4)

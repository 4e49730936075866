"""`-m gpu`: QK-norm decoders (Qwen3).  icl_qknorm_rope_kv_bf16 against the float64 norm reference of tests/qknorm_ref.py (stage 1:
every pos = 0, where the rotation is the identity and the q / k columns ARE the normed rows) and, bit for bit, against
icl_rope_kv_gqa_bf16 on a buffer holding those rows (stage 2: arbitrary positions); then a QK-norm decoder (hidden 512, 4 query /
2 K/V heads and its multi-head form, head_dim 128) through the runtime and the plugin against QKNormOracle.

Chain tolerance: the project's ratio criterion, per generated step of every row: rel(gpu, fp32 oracle) <= PARITY_RATIO x
rel(bf16-rounding oracle, fp32 oracle) — times max(1, the worst such ratio of the plain decoder of the same dims on the same
prompts), code this feature does not touch.  Both ratios are printed.

Measured on MI355X (printed by the tests, recorded in DESIGN.md): norm err / bound 1.00 at all 60 shapes (the bound is far below a
bf16 ulp, so the interval is the RNE rounding of the float64 value and an output on its end reads 1); decoder chain worst step
rel-L2 vs the bf16-rounding oracle 5.49e-3 / 5.56e-3 (grouped, 4 / 12 rows) and 5.32e-3 / 5.72e-3 (multi-head), worst step ratio
1.137 / 1.123 and 1.151 / 1.151 where the plain decoder reads 1.058 / 1.062 and 1.094 / 1.078; forward logits ratio 0.998 / 1.000;
FP8 weight mode 1.106 - 1.135."""
from dataclasses import replace

import pytest
import torch

import qknorm_ref as qr
from decoder_support import llama_oracle, row_prompts, teacher_forced_check
from fp8_ref import w_prime_state
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

PARITY_RATIO = 1.25       # the project's margin between two runs that differ only in summation order
MAX_LEN = 16
NAN = float("nan")


# ------------------------------------------------------------------------------------------------------------------
# 1. icl_qknorm_rope_kv_bf16
# ------------------------------------------------------------------------------------------------------------------
# A pass of the kernel takes 32 head rows at head_dim 128 (two per lane group: the second begins at 16) and 64 at head_dim 64
# (32); a launch with a cache has H + 2 Hkv of them.  The shapes: the ones a decoder has, and one before, on and one past 16 / 32
# (head_dim 128) and 32 / 64 (head_dim 64) head rows.
SHAPES = [(128, 4, 1), (128, 7, 1), (128, 8, 8), (128, 16, 1), (128, 32, 8),
          (128, 13, 1), (128, 14, 1), (128, 15, 1), (128, 29, 1), (128, 30, 1), (128, 31, 1),
          (64, 2, 2), (64, 16, 16), (64, 32, 1),
          (64, 29, 1), (64, 30, 1), (64, 31, 1), (64, 61, 1), (64, 62, 1), (64, 63, 1)]
PRE, GAP1, GAP2, POST = 8, 16, 8, 24          # NaN-filled columns before q, between q | k, k | v and after v


def positions(M):
    """In range, not monotonic, never 0 (test_qknorm.py runs the emulation on the same)."""
    return torch.tensor([1 + (7 * m + 3) % (MAX_LEN - 1) for m in range(M)])


class _Launch:
    """A NaN-framed QKV buffer and NaN-filled caches; run() launches the kernel under test (or icl_rope_kv_gqa_bf16) on them."""

    def __init__(self, q, k, v, n_seqs):
        self.M, self.H, self.D = q.shape
        self.Hkv = k.shape[1]
        qw, kw = self.H * self.D, self.Hkv * self.D
        self.k_off, self.v_off = qw + GAP1, qw + GAP1 + kw + GAP2               # relative to the q block
        self.full = torch.full((self.M, PRE + qw + GAP1 + kw + GAP2 + kw + POST), NAN, dtype=torch.bfloat16, device=DEV)
        self.view = self.full[:, PRE:]
        self.view[:, :qw] = q.reshape(self.M, -1).to(DEV)
        self.view[:, self.k_off:self.k_off + kw] = k.reshape(self.M, -1).to(DEV)
        self.view[:, self.v_off:self.v_off + kw] = v.reshape(self.M, -1).to(DEV)
        self.kc = torch.full((n_seqs, self.Hkv, MAX_LEN, self.D), NAN, dtype=torch.bfloat16, device=DEV)
        self.vc = torch.full_like(self.kc, NAN)
        pad = torch.ones(self.full.shape[1], dtype=torch.bool)
        for off, w in ((0, qw), (self.k_off, kw), (self.v_off, kw)):
            pad[PRE + off:PRE + off + w] = False
        self.pad = pad.to(DEV)

    def blocks(self):
        qw, kw = self.H * self.D, self.Hkv * self.D
        return (self.view[:, :qw].reshape(self.M, self.H, self.D).cpu(),
                self.view[:, self.k_off:self.k_off + kw].reshape(self.M, self.Hkv, self.D).cpu(),
                self.view[:, self.v_off:self.v_off + kw].reshape(self.M, self.Hkv, self.D).cpu())

    def run(self, B, gq, gk, cos, sin, pos, sid, norm=True):
        pos, sid = pos.to(torch.int32).to(DEV), sid.to(torch.int32).to(DEV)
        if norm:
            B.qknorm_rope_kv(self.view, self.k_off, self.v_off, gq.to(DEV), gk.to(DEV), qr.EPS, cos, sin, pos, sid, self.kc, self.vc,
                             self.H, self.Hkv, self.D, MAX_LEN)
        else:
            B.rope_kv_gqa(self.view, self.k_off, self.v_off, cos, sin, pos, sid, self.kc, self.vc, self.H, self.Hkv, self.D, MAX_LEN)
        torch.cuda.synchronize()
        return self


_worst = {}


@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("D,H,Hkv", SHAPES)
def test_qknorm_rope_kv(B, D, H, Hkv, M):
    q, k, v, gq, gk = qr.kernel_case(M, H, Hkv, D)
    cos, sin = (t.to(DEV) for t in qr.rope_tables(D, MAX_LEN))
    n_seqs = M + 2
    sid = torch.randperm(n_seqs, generator=torch.Generator().manual_seed(M + H))[:M]          # a permutation, not the identity
    name = f"qknorm_rope_kv {M}x{H}/{Hkv}x{D}"

    # stage 1: the norm alone (pos = 0: cos = 1, sin = 0, rope_rot8 returns its input)
    s1 = _Launch(q, k, v, n_seqs)
    before = s1.full.clone()
    s1.run(B, gq, gk, cos, sin, torch.zeros(M, dtype=torch.long), sid)
    n_q, n_k, v1 = s1.blocks()
    out_q, r_q = qr.norm_check(n_q, q, gq, qr.EPS)
    out_k, r_k = qr.norm_check(n_k, k, gk, qr.EPS)
    ratio = max(r_q, r_k)
    _worst[D] = max(_worst.get(D, 0.0), ratio)
    print(f"err/bound {name}: {ratio:.3f} (worst so far at head_dim {D}: {_worst[D]:.3f})")
    assert int(out_q.sum()) == 0 and int(out_k.sum()) == 0, f"{name}: {int(out_q.sum())} q / {int(out_k.sum())} k elements outside"
    bits = lambda t: t.contiguous().view(torch.int16)
    assert torch.equal(bits(v1), bits(v)), f"{name}: v columns changed"
    assert torch.equal(bits(s1.full[:, s1.pad]), bits(before[:, s1.pad])), f"{name}: padding columns changed"
    want_k = torch.full((n_seqs, Hkv, MAX_LEN, D), NAN, dtype=torch.bfloat16)
    want_v = torch.full_like(want_k, NAN)
    want_k[sid, :, 0], want_v[sid, :, 0] = n_k, v
    assert torch.equal(bits(s1.kc.cpu()), bits(want_k)), f"{name}: k cache"         # the appended rows bit for bit, NaN elsewhere
    assert torch.equal(bits(s1.vc.cpu()), bits(want_v)), f"{name}: v cache"

    # stage 2: arbitrary positions — bit-equal (+0 = -0) to icl_rope_kv_gqa_bf16 on a buffer holding stage 1's n
    pos = positions(M)
    s2 = _Launch(q, k, v, n_seqs).run(B, gq, gk, cos, sin, pos, sid)
    ref = _Launch(n_q, n_k, v, n_seqs).run(B, gq, gk, cos, sin, pos, sid, norm=False)
    assert qr.same_values(s2.full, ref.full), f"{name}: rotated q / k (or v, or the padding) differ from rope_kv_gqa on n"
    assert qr.same_values(s2.kc, ref.kc) and qr.same_values(s2.vc, ref.vc), f"{name}: caches differ from rope_kv_gqa on n"
    assert not bool(torch.isnan(s2.kc[sid.to(DEV), :, pos.to(DEV)].float()).any())

    # no cache: the same q / k, nothing else
    s3 = _Launch(q, k, v, n_seqs)
    pos_d, sid_d = pos.to(torch.int32).to(DEV), sid.to(torch.int32).to(DEV)
    B.qknorm_rope_kv(s3.view, s3.k_off, s3.v_off, gq.to(DEV), gk.to(DEV), qr.EPS, cos, sin, pos_d, sid_d, None, None, H, Hkv, D, 0)
    assert qr.same_values(s3.full, s2.full), f"{name}: the launch without caches differs"


def test_qknorm_argument_checks(B):
    D, H, Hkv, M = 128, 4, 2, 2
    buf = torch.zeros(M, (H + 2 * Hkv) * D, dtype=torch.bfloat16, device=DEV)
    g = torch.ones(D, device=DEV)
    cos, sin = (t.to(DEV) for t in qr.rope_tables(D, MAX_LEN))
    z = torch.zeros(M, dtype=torch.int32, device=DEV)
    kc = torch.zeros(M, Hkv, MAX_LEN, D, dtype=torch.bfloat16, device=DEV)
    k_off, v_off = H * D, (H + Hkv) * D
    B.qknorm_rope_kv(buf, k_off, v_off, g, g, qr.EPS, cos, sin, z, torch.arange(M, dtype=torch.int32, device=DEV), kc, kc.clone(),
                     H, Hkv, D, MAX_LEN)                                                           # the valid call
    bad = [dict(q_gamma=None), dict(k_gamma=None),                                                 # NULL gamma
           dict(head_dim=96),                                                                      # head_dim 96
           dict(n_kv_heads=3),                                                                     # 4 % 3
           dict(k_off=k_off - 8), dict(v_off=v_off - 8),                                           # overlapping column blocks
           dict(vcache=None), dict(kcache=None)]                                                   # one cache NULL
    for kw in bad:
        a = dict(k_off=k_off, v_off=v_off, q_gamma=g, k_gamma=g, kcache=kc, vcache=kc, n_kv_heads=Hkv, head_dim=D)
        a.update(kw)
        with pytest.raises(B.IclError):
            B.qknorm_rope_kv(buf, a["k_off"], a["v_off"], a["q_gamma"], a["k_gamma"], qr.EPS, cos, sin, z, z, a["kcache"], a["vcache"],
                             H, a["n_kv_heads"], a["head_dim"], MAX_LEN)


# ------------------------------------------------------------------------------------------------------------------
# 2. the QK-norm decoder through the runtime
# ------------------------------------------------------------------------------------------------------------------
LENS = {"4rows": [33, 90, 61, 12], "12rows": [33, 90, 61, 12, 5, 70, 44, 21, 9, 57, 28, 16]}      # test_gpu_gqa.test_decoder_chain


def _llama(base, kv, qk_norm=True, **kw):
    return replace(base, hidden=512, n_layers=2, n_heads=4, n_kv_heads=kv, ffn=1024, qk_norm=qk_norm, **kw)


class _Env:
    def __init__(self, kv, qk_norm=True, **rt_kw):
        from icl_speech_text_llm_amd.runtime import synth
        from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
        from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
        tiny = SalmonnCfg.tiny(use_beats=False)
        self.cfg = replace(tiny, llama=_llama(tiny.llama, kv, qk_norm))
        self.sd = synth.salmonn_state(self.cfg, seed=0, jitter=True, parts=("llama",))
        self.rt = SalmonnRuntime(self.cfg, dict(self.sd), device=DEV, parts=("llama",), **rt_kw)


@pytest.fixture(scope="module", params=[2, None], ids=["gqa", "mha"])
def env(request):
    return _Env(request.param)


_plain_envs, _plain_ratios = {}, {}


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _step_ratios(rt, ob_b, ob_f, prompts, tag):
    """Worst, over the rows and the 10 steps, of rel(gpu, fp32 oracle) / rel(bf16-rounding oracle, fp32 oracle), both oracles
    teacher-forced along the GPU's own tokens; also the worst rel(gpu, bf16-rounding oracle)."""
    res = rt.generate(prompts, None, max_new_tokens=10, suppress_eos=True, want_step_logits=True)
    worst, worst_b = 0.0, 0.0
    for i, segs in enumerate(prompts):
        toks = res.tokens[i][None]
        ids = torch.tensor(segs[0])
        tf_b = ob_b.teacher_forced_logits(ob_b.embed(ids)[None], toks)[0]
        tf_f = ob_f.teacher_forced_logits(ob_f.embed(ids)[None], toks)[0]
        g = res.step_logits[:, i].float().cpu()
        for t in range(10):
            worst = max(worst, _rel(g[t], tf_f[t]) / _rel(tf_b[t], tf_f[t]))
            worst_b = max(worst_b, _rel(g[t], tf_b[t]))
    print(f"{tag}: worst step rel-L2 vs the bf16-rounding oracle {worst_b:.3e}; worst step ratio rel(gpu, fp32) / rel(bf16 oracle, fp32) {worst:.3f}")
    return worst


def _plain_ratio(kv, which):
    """The same ratio of the plain decoder of the same dims (qk_norm=False) on the same prompts, once per (heads, rows)."""
    if (kv, which) not in _plain_ratios:
        if kv not in _plain_envs:
            _plain_envs[kv] = _Env(kv, qk_norm=False)
        p = _plain_envs[kv]
        prompts = row_prompts(p.cfg.llama.vocab, LENS[which], seed=7)
        _plain_ratios[kv, which] = _step_ratios(p.rt, llama_oracle(p.sd, p.cfg.llama), llama_oracle(p.sd, p.cfg.llama, rnd=False), prompts,
                                                f"plain decoder kv={kv} {which}")
    return _plain_ratios[kv, which]


@pytest.mark.parametrize("which", ["4rows", "12rows"])
def test_decoder_chain(env, which):
    """Prefill + 10 decode steps, teacher-forced against QKNormOracle: the token criteria of teacher_forced_check (2x / 4x the
    step's own error) and the ratio criterion of the module docstring at every step of every row."""
    c = env.cfg.llama
    assert c.qk_norm and env.rt.llama.w.layers[0].q_gamma.shape == (128,)
    prompts = row_prompts(c.vocab, LENS[which], seed=7)
    ob_b, ob_f = llama_oracle(env.sd, c), llama_oracle(env.sd, c, rnd=False)
    tag = f"qk-norm decoder kv={c.n_kv_heads} {which}"
    e = teacher_forced_check(env.rt, ob_b, prompts, tag)
    print(f"{tag}: worst step rel-L2 (teacher-forced check) {e:.3e}")
    ratio = _step_ratios(env.rt, ob_b, ob_f, prompts, tag)
    plain = _plain_ratio(c.n_kv_heads, which)
    print(f"{tag}: ratio {ratio:.3f}, plain decoder {plain:.3f}, allowed {PARITY_RATIO * max(1.0, plain):.3f}")
    assert ratio <= PARITY_RATIO * max(1.0, plain)


def test_forward_logits_graph_chunks_and_sampling(env):
    """The same model through the other paths: teacher-forced forward (no cache) under the ratio criterion; captured-graph
    decode and chunked prefill torch.equal to the eager / unchunked run; a seeded sampled run repeats."""
    c, rt = env.cfg.llama, env.rt
    prompts = row_prompts(c.vocab, [37, 150, 64], seed=3)
    ob_b, ob_f = llama_oracle(env.sd, c), llama_oracle(env.sd, c, rnd=False)
    fwd = lambda ob: torch.cat([ob.forward(ob.embed(torch.tensor(p[0]))[None])[0][0] for p in prompts])
    want_b, want_f = fwd(ob_b), fwd(ob_f)
    got, n = rt.forward_logits(prompts, None)
    got = got.float().cpu()
    ratio = _rel(got, want_f) / _rel(want_b, want_f)
    if c.n_kv_heads not in _plain_envs:
        _plain_envs[c.n_kv_heads] = _Env(c.n_kv_heads, qk_norm=False)
    p = _plain_envs[c.n_kv_heads]
    pb, pf = llama_oracle(p.sd, p.cfg.llama), llama_oracle(p.sd, p.cfg.llama, rnd=False)
    fwd_p = lambda ob: torch.cat([ob.forward(ob.embed(torch.tensor(q[0]))[None])[0][0] for q in prompts])
    plain_f = fwd_p(pf)
    plain = _rel(p.rt.forward_logits(prompts, None)[0].float().cpu(), plain_f) / _rel(fwd_p(pb), plain_f)
    print(f"forward logits kv={c.n_kv_heads}: rel-L2 vs bf16 oracle {_rel(got, want_b):.3e}, vs fp32 {_rel(got, want_f):.3e}, "
          f"ratio {ratio:.3f}, plain decoder {plain:.3f}")
    assert n == [37, 150, 64] and ratio <= PARITY_RATIO * max(1.0, plain)

    # captured-graph decode == eager
    rt._graphs.clear(); rt._graph_warm.clear()
    lens = [21, 40, 33]
    outs = [rt.generate(row_prompts(c.vocab, lens, seed=s), None, max_new_tokens=8, suppress_eos=True).tokens.clone() for s in (11, 12, 13, 11)]
    assert len(rt._graphs) == 1 and torch.equal(outs[0], outs[3])
    rt.use_graphs = False
    try:
        eager = rt.generate(row_prompts(c.vocab, lens, seed=13), None, max_new_tokens=8, suppress_eos=True).tokens
    finally:
        del rt.use_graphs
    assert torch.equal(eager, outs[2])

    # chunked prefill == unchunked
    many = row_prompts(c.vocab, [37, 64, 5, 50, 21, 44, 9], seed=4100)
    try:
        rt.prefill_chunk = 128
        want = rt.generate(many, None, max_new_tokens=6, suppress_eos=True, want_first_logits=True)
        want_tok, want_first = want.tokens.clone(), want.first_logits.clone()
        for chunk in (1, 3):
            rt.prefill_chunk = chunk
            res = rt.generate(many, None, max_new_tokens=6, suppress_eos=True, want_first_logits=True)
            assert torch.equal(res.first_logits, want_first) and torch.equal(res.tokens, want_tok), f"chunk {chunk}"
    finally:
        del rt.prefill_chunk

    # a seeded sampled run repeats
    outs = [rt.generate(prompts, None, max_new_tokens=6, do_sample=True, temperature=0.8, top_p=0.9, suppress_eos=True,
                        generator=torch.Generator(device=DEV).manual_seed(5)).tokens for _ in range(2)]
    assert outs[0].shape == (3, 6) and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("kv", [2, None], ids=["gqa", "mha"])
def test_margin_weights_beam(kv):
    """Decisive-margin weights: num_beams=3 returns the oracle's beam ids (as test_gpu_gqa.test_margin_weights_greedy_and_beam)."""
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    tiny = SalmonnCfg.tiny(use_beats=False)
    cfg = replace(tiny, llama=_llama(tiny.llama, kv))
    sd = synth.salmonn_state(cfg, seed=1, parts=("llama",), margin=True)
    rt = SalmonnRuntime(cfg, dict(sd), device=DEV, parts=("llama",))
    prompts = row_prompts(cfg.llama.vocab, [33, 90, 61], seed=21)
    beams = rt.generate(prompts, None, max_new_tokens=5, suppress_eos=True, num_beams=3)
    ob = llama_oracle(sd, cfg.llama)
    for b, p in enumerate(prompts):
        want = ob.generate_beam(ob.embed(torch.tensor(p[0]))[None], 5, -1, cfg.llama.pad_id, 3, 1.0)
        assert beams.tokens[b, :want.shape[1]].tolist() == want[0].tolist(), b


def test_fp8_weight_mode(env):
    """llm_weight_dtype="fp8" with QK-norm at 4 rows (the fp8-weight skinny kernel) and 12 rows (the bf16 tiles on W'), against
    the oracle given W', under the same criteria."""
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    c = env.cfg.llama
    r8 = SalmonnRuntime(env.cfg, dict(env.sd), device=DEV, parts=("llama",), llm_weight_dtype="fp8")
    wsd = w_prime_state(env.sd, c)
    assert all(torch.equal(wsd[k], env.sd[k]) for k in wsd if k.endswith("_norm.weight"))
    ob_b, ob_f = llama_oracle(wsd, c), llama_oracle(wsd, c, rnd=False)
    for which in ("4rows", "12rows"):
        prompts = row_prompts(c.vocab, LENS[which], seed=7)
        tag = f"fp8 weight mode, qk-norm kv={c.n_kv_heads} {which}"
        teacher_forced_check(r8, ob_b, prompts, tag)
        ratio = _step_ratios(r8, ob_b, ob_f, prompts, tag)
        plain = _plain_ratio(c.n_kv_heads, which)
        print(f"{tag}: ratio {ratio:.3f}, plain decoder {plain:.3f}")
        assert ratio <= PARITY_RATIO * max(1.0, plain)


def test_fp8_kv_is_refused_before_any_launch(env):
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    with pytest.raises(ValueError, match="QK-norm|grouped-query"):
        SalmonnRuntime(env.cfg, dict(env.sd), device=DEV, parts=("llama",), llm_kv_dtype="fp8")


# ------------------------------------------------------------------------------------------------------------------
# 3. the plugin on a Qwen3 HF folder
# ------------------------------------------------------------------------------------------------------------------
def test_plugin_loads_a_qwen3_hf_folder(tmp_path):
    """CustomSALMONN(llama_path=<folder saved by Qwen3ForCausalLM.save_pretrained>) loads the per-head gains and generates; the
    same folder declared as model_type "llama" is refused by name of the stray key."""
    import json
    import shutil
    from transformers import Qwen3Config, Qwen3ForCausalLM, WhisperConfig, WhisperModel
    from icl_speech_text_llm_amd.models.custom_salmon import CustomSALMONN
    from icl_speech_text_llm_amd.models.model_factory import ModelFactory
    from icl_speech_text_llm_amd.utils.tokenization import ByteTokenizer
    from oracle import models as om
    torch.manual_seed(0)
    llama = Qwen3ForCausalLM(Qwen3Config(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                         head_dim=128, intermediate_size=1024, vocab_size=259, rms_norm_eps=1e-6,
                                         max_position_embeddings=2048, tie_word_embeddings=False, bos_token_id=1,
                                         eos_token_id=2)).eval()
    whisper = WhisperModel(WhisperConfig(d_model=128, encoder_layers=2, encoder_attention_heads=2, encoder_ffn_dim=256,
                                         decoder_layers=1, decoder_attention_heads=2, decoder_ffn_dim=64, num_mel_bins=80,
                                         max_source_positions=1500, vocab_size=64, pad_token_id=0, bos_token_id=1, eos_token_id=2,
                                         decoder_start_token_id=1)).eval()
    with torch.no_grad():
        for name, p in llama.named_parameters():
            if p.dim() > 1:
                p.mul_(3.0)                                         # away from the N(0, 0.02) near-degenerate regime
            elif name.endswith(("q_norm.weight", "k_norm.weight")):
                p.add_(0.3 * torch.randn_like(p))
    llama.save_pretrained(tmp_path / "llama", safe_serialization=True)
    whisper.save_pretrained(tmp_path / "whisper", safe_serialization=True)
    kw = dict(whisper_path=str(tmp_path / "whisper"), beats_path="", lora=False, ckpt_path="", device=DEV)
    m = CustomSALMONN(llama_path=str(tmp_path / "llama"), tokenizer=ByteTokenizer(260), **kw).eval()
    c = m.cfg.llama
    assert (c.hidden, c.n_heads, c.n_kv_heads, c.head_dim, c.vocab, c.qk_norm, c.rms_eps) == (512, 4, 2, 128, 260, True, 1e-6)
    hf_sd = {k: v.detach().float() for k, v in llama.state_dict().items()}
    key = "model.layers.1.self_attn.k_norm.weight"
    assert torch.equal(m.salmonn.state_dict()["llama_model." + key].float().cpu(), hf_sd[key])
    prompts = ["classify this sentence please.\nOutput:", "is it positive?\nOutput:", "short\nOutput:"]
    batch = {"prompt": prompts, "num_examples": torch.tensor([0, 0, 0]), "max_new_tokens": 6}
    texts = m.generate_output(dict(batch))
    assert isinstance(texts, list) and len(texts) == 3 and all(isinstance(t, str) for t in texts)
    res = m.generate_ids(dict(batch), want_first_logits=True)
    ob = qr.QKNormOracle(hf_sd, 4, 1e-6, rope_theta=c.rope_theta, rnd=om.bf16_round, n_kv_heads=2)
    for b, prompt in enumerate(prompts):
        ids = m.llama_tokenizer(prompt, add_special_tokens=False, return_tensors="pt")["input_ids"]
        _, first = ob.generate_greedy(ob.embed(ids[0])[None], 1, -1, 259, return_first_logits=True)
        got, first = res.first_logits[b, :259].float().cpu(), first[0]
        err = float((got - first).abs().max())
        top2 = first.topk(2)
        chosen = int(res.tokens[b, 0])
        print(f"plugin qwen3 row {b}: first-logit max abs err {err:.2e}, oracle margin {float(top2.values[0] - top2.values[1]):.2e}")
        assert float(top2.values[0] - first[chosen]) <= 2 * err + 1e-6
        if float(top2.values[0] - top2.values[1]) > 4 * err:
            assert chosen == int(top2.indices[0])
    # the same tensors under model_type "llama": the two gains would be dropped — refused, through the factory's wrapped error
    shutil.copytree(tmp_path / "llama", tmp_path / "as_llama")
    cj = json.loads((tmp_path / "as_llama" / "config.json").read_text())
    cj["model_type"] = "llama"
    (tmp_path / "as_llama" / "config.json").write_text(json.dumps(cj))
    with pytest.raises(RuntimeError, match=r"Failed to create model: .*self_attn\.[qk]_norm\.weight") as ei:
        ModelFactory.create_model("salmonn", llama_path=str(tmp_path / "as_llama"), tokenizer=ByteTokenizer(260), **kw)
    assert isinstance(ei.value.__cause__, ValueError)


def test_qwen_runtime_with_a_qk_norm_llm():
    """QwenAudioCfg.llm carries qk_norm too (q / k / v biases in front of the norm, LoRA on q and k): forward logits against
    QKNormOracle under the ratio criterion, and a short greedy run."""
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import QwenAudioCfg
    from icl_speech_text_llm_amd.runtime.qwen import QwenAudioRuntime
    q = QwenAudioCfg.tiny()
    prompts = row_prompts(q.llm.vocab - 1, [37, 150, 64], seed=9)            # below the audio token id
    ratios = {}
    for qk_norm in (True, False):
        cfg = replace(q, llm=_llama(q.llm, 2, qk_norm))
        assert cfg.llm.qkv_bias and cfg.llm.lora_targets == ("q_proj", "k_proj")
        sd = synth.qwen_audio_state(cfg, seed=0)
        assert ("language_model.model.layers.0.self_attn.k_norm.weight" in sd) == qk_norm
        rt = QwenAudioRuntime(cfg, dict(sd), device=DEV)
        ob_b, ob_f = (llama_oracle(sd, cfg.llm, "language_model.", rnd) for rnd in (True, False))
        fwd = lambda ob: torch.cat([ob.forward(ob.embed(torch.tensor(p[0]))[None])[0][0] for p in prompts])
        want_b, want_f = fwd(ob_b), fwd(ob_f)
        got = rt.forward_logits(prompts, None)[0].float().cpu()
        ratios[qk_norm] = _rel(got, want_f) / _rel(want_b, want_f)
        print(f"qwen forward logits qk_norm={qk_norm}: rel-L2 vs bf16 oracle {_rel(got, want_b):.3e}, ratio {ratios[qk_norm]:.3f}")
        if qk_norm:
            assert rt.generate(prompts, None, max_new_tokens=4, suppress_eos=True).tokens.shape == (3, 4)
    assert ratios[True] <= PARITY_RATIO * max(1.0, ratios[False])

"""`-m gpu`: the prompt-attention readout.  icl_attn_segmass_bf16 against the float64 reference of tests/attn_segmass_ref.py, per
element of mass and probs (the bound and its derivation are in that module's docstring; tests/test_attn_segmass_ref.py shows on the
CPU that it admits an f32 emulation and rejects five one-key mutants on the cases used here), with a count and a peak probe, batch
invariance and reproducibility bit for bit; then ``prompt_attention`` of the runtime (multi-head: the trimmed last layer; grouped;
QK-norm on and off) against its own probs, ``generate``'s first logits and transformers' eager attention; then the plugin.

Every launch covers lens 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65 and 385 at max_len 448, NaN in the cache rows and 0xFF in the
segment bytes past each length.  Which test reaches which instantiation:
  test_kernel[D64-H3|4-...]      attn_segmass_kernel<64, 1>   (tiles of 128 keys: 385 = 3 tiles + 1 key)
  test_kernel[D128-H3|4-kv=H]    attn_segmass_kernel<128, 1>  (tiles of 64 keys: 385 = 6 tiles + 1 key)
  test_kernel[D128-H2G-kv2]      attn_segmass_kernel<128, G>, G = 2, 4, 7, 8

HF comparison (test_runtime): rel-L2 of the per-segment mass over all rows, layers and heads against the same transformers model
in fp32 on the CPU; allowed: 1.25 x the rel-L2 of that model run in bf16 against itself in fp32 (the project's ratio criterion).
Both figures are printed.

Measured on MI355X (printed by the tests, recorded in README.md): largest err / bound, mass | probs — random data 0.004 | 0.006
(head_dim 64), 0.002 | 0.002 (128), 0.002 | 0.003 (grouped); count probe 0.019 | 0.001, 0.010 | 0.000, 0.010 | 0.000; peak probe
0.515 | 0.515 (64) and 0.707 | 0.707 (128, grouped): its far keys, whose weights lie below 2^-126 and are held to the bound's
absolute term.  Mass against HF fp32, rel-L2, next to HF bf16 against HF fp32: multi-head 6.08e-4 / 1.07e-3 (ratio 0.57), grouped
6.50e-4 / 1.02e-3 (0.64), grouped QK-norm 3.42e-3 / 6.26e-3 (0.55), multi-head QK-norm 3.37e-3 / 6.40e-3 (0.53).
"""
import pytest
import torch

import attn_segmass_ref as sr
import probe_harness as ph
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _launch(B, q, kc, lens, seg, n_seg, H, Hkv, D, *, probs=True, q_rows=None):
    """One launch on device copies; mass and probs start as NaN, Q is a column slice of a wider buffer.  Returns CPU tensors."""
    n = len(lens)
    qbuf = torch.full((q.shape[0], H * D + 64), NAN, dtype=torch.bfloat16, device=DEV)
    qbuf[:, 32:32 + H * D] = q.to(DEV)
    mass = torch.full((n, H, n_seg), NAN, device=DEV)
    pr = torch.full((n, H, kc.shape[2] + 8), NAN, device=DEV) if probs else None
    B.attn_segmass(qbuf[:, 32:32 + H * D], kc.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), seg.to(DEV), mass, H, D,
                   kc.shape[2], D ** -0.5, n_kv_heads=Hkv, q_rows=None if q_rows is None else q_rows.to(DEV), probs=pr)
    torch.cuda.synchronize()
    return mass.cpu(), None if pr is None else pr.cpu()


def _assert_bound(mass, probs, R, D, what):
    rm, rp = sr.mass_ratio(mass, R, D), sr.probs_ratio(probs[:, :, :R.probs.shape[2]], R, D)
    print(f"err/bound {what}: mass {float(rm.max()):.3f}, probs {float(rp.max()):.3f}")
    assert float(rm.max()) <= 1, f"{what}: mass err/bound {float(rm.max()):.3g} at {sr.describe(rm)}"
    assert float(rp.max()) <= 1, f"{what}: probs err/bound {float(rp.max()):.3g} at {sr.describe(rp)}"
    dead = ~R.live[:, None, :].expand(-1, probs.shape[1], -1)
    assert bool(torch.isnan(probs[:, :, :R.probs.shape[2]][dead]).all()) and bool(torch.isnan(probs[:, :, R.probs.shape[2]:]).all()), \
        f"{what}: probs written at or past a length"
    empty = (R.n_g == 0)[:, None, :].expand_as(mass)
    assert bool((mass[empty] == 0).all()), f"{what}: a segment without a key is not exactly 0"
    return float(rm.max()), float(rp.max())


@pytest.mark.parametrize("case", sr.CASES, ids=sr.case_id)
def test_kernel(B, case):
    D, H, Hkv, n_seg = case
    lens, scale = list(sr.LENS), D ** -0.5
    seg = sr.make_seg(lens, n_seg)
    name = f"attn_segmass {sr.case_id(case)}"

    # random data against the bound; the masses sum to the reference's partial sum (ignored ids inside every longer row)
    q, kc = sr.random_case(lens, H, Hkv, D)
    R = sr.reference(q, kc, lens, seg, n_seg, H, Hkv, D, scale)
    mass, probs = _launch(B, q, kc, lens, seg, n_seg, H, Hkv, D)
    _assert_bound(mass, probs, R, D, f"{name} normal")
    total_rel = sr.C1 * D * sr.U * R.S + sr.C2 * (2 * R.n[:, None] + 8) * sr.U          # n_g <= n in every term of the sum
    assert bool(((mass.double().sum(-1) - R.mass.sum(-1)).abs() <= R.mass.sum(-1) * total_rel + R.n[:, None] * sr.TINY).all())
    assert float((R.mass.sum(-1) - 1).abs().max()) > 1e-3
    # without probs: the same mass bits; q_rows: a permuted Q buffer gives the same bits
    assert torch.equal(_launch(B, q, kc, lens, seg, n_seg, H, Hkv, D, probs=False)[0], mass), f"{name}: probs=NULL changes mass"
    perm = torch.randperm(len(lens), generator=torch.Generator().manual_seed(3))
    wide = torch.full((len(lens) + 3, H * D), NAN, dtype=torch.bfloat16)
    wide[perm] = q
    m2, p2 = _launch(B, wide, kc, lens, seg, n_seg, H, Hkv, D, q_rows=perm.to(torch.int32))
    assert torch.equal(m2, mass) and torch.equal(p2.nan_to_num(-1.0), probs.nan_to_num(-1.0)), f"{name}: q_rows"
    # two launches give equal bits
    m3, p3 = _launch(B, q, kc, lens, seg, n_seg, H, Hkv, D)
    assert torch.equal(m3, mass) and torch.equal(p3.nan_to_num(-1.0), probs.nan_to_num(-1.0)), f"{name}: not reproducible"

    # count probe: probs = 1 / n, mass_g = n_g / n
    q, kc = sr.count_probe(lens, H, Hkv, D)
    R = sr.reference(q, kc, lens, seg, n_seg, H, Hkv, D, scale)
    assert float((R.mass - (R.n_g / R.n[:, None])[:, None, :]).abs().max()) < 1e-13
    mass, probs = _launch(B, q, kc, lens, seg, n_seg, H, Hkv, D)
    _assert_bound(mass, probs, R, D, f"{name} count probe")

    # peak probe: the target's segment holds the mass (the reference says so first), every other segment next to nothing
    q, kc, tgt = sr.peak_probe(lens, H, Hkv, D, seg, n_seg)
    R = sr.reference(q, kc, lens, seg, n_seg, H, Hkv, D, scale)
    mass, probs = _launch(B, q, kc, lens, seg, n_seg, H, Hkv, D)
    _assert_bound(mass, probs, R, D, f"{name} peak probe")
    for b in range(len(lens)):
        for h in range(H):
            t = int(tgt[b, h])
            g = int(seg[b, t])
            rel = sr.C1 * D * sr.U * float(R.S[b, h]) + sr.C2 * (2 * lens[b] + 8) * sr.U      # the bound's relative part at n_g = n
            assert float(R.probs[b, h, t]) >= sr.W_EXACT
            assert float(probs[b, h, t]) >= sr.W_EXACT * (1 - rel), f"{name} peak probe: row {b} head {h} key {t}"
            if g < n_seg:
                assert float(R.mass[b, h, g]) >= sr.W_EXACT and float(mass[b, h, g]) >= sr.W_EXACT * (1 - rel), \
                    f"{name} peak probe: row {b} head {h} key {t} segment {g}"


@pytest.mark.parametrize("D,H,Hkv", [(128, 4, 4), (64, 4, 4), (128, 8, 2)], ids=["D128", "D64", "gqa4"])
def test_batch_invariance(B, D, H, Hkv):
    """Every row alone gives the bits it gives in a batch of 12 (48 / 24 workgroups) and in one of 264 (more than 1024 at 4 K/V
    heads; 528 grouped)."""
    lens, n_seg = list(sr.LENS), 32
    seg = sr.make_seg(lens, n_seg)
    q, kc = sr.random_case(lens, H, Hkv, D)
    mass, probs = _launch(B, q, kc, lens, seg, n_seg, H, Hkv, D)
    for b, L in enumerate(lens):
        m1, p1 = _launch(B, q[b:b + 1], kc[b:b + 1], [L], seg[b:b + 1], n_seg, H, Hkv, D)
        assert torch.equal(m1[0], mass[b]) and torch.equal(p1[0, :, :L], probs[b, :, :L]), f"row {b} (len {L}) alone != in the batch"
    reps = 22
    assert len(lens) * reps * Hkv > 1024 or Hkv < 4
    mb, pb = _launch(B, q.repeat(reps, 1), kc.repeat(reps, 1, 1, 1), lens * reps, seg.repeat(reps, 1), n_seg, H, Hkv, D)
    assert torch.equal(mb, mass.repeat(reps, 1, 1)) and torch.equal(pb.nan_to_num(-1.0), probs.repeat(reps, 1, 1).nan_to_num(-1.0))


def test_binding_refuses_what_the_entry_point_refuses(B):
    D, H = 128, 4
    q, kc = sr.random_case([5, 9], H, H, D, max_len=16)
    seg = sr.make_seg([5, 9], 2, max_len=16)
    _launch(B, q, kc, [5, 9], seg, 2, H, H, D)                                       # the valid call
    args = lambda **kw: dict(dict(q=q.to(DEV), kc=kc.to(DEV), n_seg=2, Hkv=0, D=D, scale=D ** -0.5, seg=seg.to(DEV)), **kw)
    for kw in (dict(n_seg=33), dict(D=96), dict(Hkv=3), dict(scale=float("inf")), dict(seg=seg[:, :15].contiguous().to(DEV))):
        a = args(**kw)
        mass = torch.zeros(2, H, a["n_seg"], device=DEV)
        with pytest.raises(B.IclError, match="icl_attn_segmass_bf16"):
            B.attn_segmass(a["q"], a["kc"], torch.tensor([5, 9], dtype=torch.int32, device=DEV), a["seg"], mass, H, a["D"], 16,
                           a["scale"], n_kv_heads=a["Hkv"])


# ------------------------------------------------------------------------------------------------------------------
# the runtime
# ------------------------------------------------------------------------------------------------------------------
class _Env(ph.Decoder):
    """The 2-layer decoder of tests/probe_harness.py on the GPU, with the ``synth.salmonn_state`` weights as they are."""

    def __init__(self, kv, qk_norm):
        super().__init__(kv, qk_norm, n_layers=2, redraw=False, speech_scale=0.05)
        self.rt = self.runtime(DEV)
        self.segments = [ph.four_runs(n, {n // 2: 255}) for n in ph.PROMPT_LENS]        # four runs with one position ignored
        self.segments[ph.SPEECH_ROW] = ph.speech_row_runs()
        self.n_seg = 4

    def hf_mass(self, m, dtype):
        """[B, n_layers, n_heads, n_seg] float64: the last query row of transformers' eager attention, summed per segment."""
        m, c = m.to(dtype), self.cfg.llama
        emb = m.get_input_embeddings().weight.detach().float()
        out = torch.zeros(len(self.prompts), c.n_layers, c.n_heads, self.n_seg, dtype=torch.float64)
        for b, segs in enumerate(self.prompts):
            x = torch.cat([self.speech[s[1]:s[1] + s[2]] if isinstance(s, tuple) else emb[torch.tensor(s)] for s in segs])
            with torch.no_grad():
                att = m(inputs_embeds=x[None].to(dtype), output_attentions=True).attentions
            ids = torch.tensor(self.segments[b])
            for l, a in enumerate(att):
                last = a[0, :, -1, :].double()                                                # [H, S]
                for g in range(self.n_seg):
                    out[b, l, :, g] = last[:, ids == g].sum(-1)
        return out


@pytest.fixture(scope="module", params=[(None, False), (2, False), (2, True), (None, True)], ids=["mha", "gqa", "gqa-qknorm", "mha-qknorm"])
def env(request):
    return _Env(*request.param)


def test_runtime(env):
    rt, c = env.rt, env.cfg.llama
    sp = env.speech.to(DEV)
    res = rt.prompt_attention(env.prompts, sp, env.segments, want_probs=True)
    lens = res.lens
    assert lens == env.lens
    assert res.mass.shape == (len(lens), c.n_layers, c.n_heads, env.n_seg) and res.mass.device.type == "cpu"
    assert res.probs.shape[:3] == (len(lens), c.n_layers, c.n_heads) and res.probs.shape[3] >= max(lens)
    # first logits: generate's, bit for bit (and again after the readout: the default path is undisturbed)
    gen = rt.generate(env.prompts, sp, max_new_tokens=1, suppress_eos=True, want_first_logits=True)
    assert torch.equal(res.first_logits, gen.first_logits)
    assert torch.equal(rt.generate(env.prompts, sp, max_new_tokens=3, suppress_eos=True, want_first_logits=True).first_logits,
                       gen.first_logits)
    # without probs, and in chunks of two sequences: the same mass bits
    assert torch.equal(rt.prompt_attention(env.prompts, sp, env.segments).mass, res.mass)
    with ph.prefill_chunks(rt, 2):
        chunked = rt.prompt_attention(env.prompts, sp, env.segments, want_probs=True)
    assert torch.equal(chunked.mass, res.mass) and torch.equal(chunked.probs, res.probs) and torch.equal(chunked.first_logits, res.first_logits)
    # every layer's mass is the segmented sum of its probs: float64 recomputation, the f32 sum bound c2 * n_g * u of the reference module
    probs = res.probs.double().cpu()
    for b, n in enumerate(lens):
        ids = torch.tensor(env.segments[b])
        assert float((probs[b, :, :, :n].sum(-1) - 1).abs().max()) < 1e-4 and bool((probs[b, :, :, n:] == 0).all())
        for g in range(env.n_seg):
            want = probs[b, :, :, :n][:, :, ids == g].sum(-1)
            n_g = int((ids == g).sum())
            assert bool(((res.mass[b, :, :, g].double() - want).abs() <= want * sr.C2 * n_g * sr.U + n_g * sr.TINY).all()), (b, g)
    # transformers' eager attention on the same weights, fp32 on the CPU; the reference's own rounding: the same model in bf16
    hf = env.hf()
    want32 = env.hf_mass(hf, torch.float32)
    want16 = env.hf_mass(hf, torch.bfloat16)
    own, got = ph.rel(want16, want32), ph.rel(res.mass.double(), want32)
    print(f"prompt_attention kv={c.n_kv_heads} qk_norm={c.qk_norm}: rel-L2 of mass vs HF fp32 {got:.3e}; HF bf16 vs HF fp32 {own:.3e}; "
          f"ratio {got / own:.3f} (allowed {ph.PARITY_RATIO})")
    assert got <= ph.PARITY_RATIO * own


def test_runtime_refusals(env):
    rt, c = env.rt, env.cfg.llama
    sp = env.speech.to(DEV)
    before = rt.ws.nbytes()
    with pytest.raises(ValueError, match="positions"):                       # a segment list of the wrong length
        rt.prompt_attention(env.prompts, sp, [s[:-1] for s in env.segments])
    with pytest.raises(ValueError, match="segment lists"):
        rt.prompt_attention(env.prompts, sp, env.segments[:-1])
    with pytest.raises(ValueError, match="at most 32"):                      # more than 32 segments
        rt.prompt_attention(env.prompts[:1], None, [list(range(33))])
    with pytest.raises(ValueError, match="max_pos"):                         # a prompt over max_pos
        rt.prompt_attention([[[5] * (c.max_pos + 1)]], None, [[0] * (c.max_pos + 1)])
    assert rt.ws.nbytes() == before                                          # nothing was sized, nothing launched
    if c.group == 1 and not c.qk_norm:                                       # the FP8 KV cache exists for this form only
        r8 = env.runtime(DEV, llm_kv_dtype="fp8")
        with pytest.raises(ValueError, match="bf16 KV cache"):
            r8.prompt_attention(env.prompts, sp, env.segments)


# ------------------------------------------------------------------------------------------------------------------
# the plugin
# ------------------------------------------------------------------------------------------------------------------
def test_plugin():
    model, b = ph.tiny_plugin_batches(2)
    out = model.prompt_attention(dict(b))
    assert set(out) == {"mass", "pieces", "first_logits"}
    c = model.cfg.llama
    n_pieces = max(len(p) for p in out["pieces"])
    assert out["mass"].shape == (2, c.n_layers, c.n_heads, n_pieces) and out["first_logits"].shape == (2, c.vocab)
    for pc in out["pieces"]:
        kinds = [k for k, _ in pc]
        assert kinds.count("example") == 2 and kinds.count("speech") == 1 and [e for e in pc if e[0] == "example"] == [("example", 0), ("example", 1)]
        assert kinds.index("speech") > max(i for i, k in enumerate(kinds) if k == "example")
    # every position lies in a piece, so each (layer, head) sums to 1: n keys of relative error c1 D u S + c2 (2 n + 8) u each, S
    # taken at its cap for bf16 unit-scale rows of this model (|s| <= 64) — far below the 1e-4 a lost key of weight 1 / n would cost
    n = 1024
    tol = sr.C1 * c.head_dim * sr.U * 64 + sr.C2 * (2 * n + 8) * sr.U
    assert float((out["mass"].double().sum(-1) - 1).abs().max()) <= tol, float((out["mass"].double().sum(-1) - 1).abs().max())
    assert bool((out["mass"] >= 0).all())
    res = model.generate_ids(dict(b), want_first_logits=True)
    assert torch.equal(out["first_logits"], res.first_logits)
    with pytest.raises(ValueError, match="row 0"):
        model.MAX_PIECES = 3
        try:
            model.prompt_attention(dict(b))
        finally:
            del model.MAX_PIECES

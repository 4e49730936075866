"""`-m gpu`: ``prompt_attention(..., want_flow=True)`` of the runtime and ``prompt_attention(samples, flow=True)`` of the plugin.

2-layer decoders of tests/probe_harness.py (hidden 512, 4 heads of 128; no LoRA, so a transformers model holds the same tensors)
over five ragged prompts of text:
multi-head — whose last layer a plain call trims to the last rows, and a flow call keeps at full height — and grouped 4 / 2 with
QK-norm.  Bit for bit: with ``want_flow``, ``first_logits`` and ``mass`` are those of the call without it and ``first_logits`` are
``generate``'s; prefill chunks of two sequences give the bits of one chunk.  Within the two kernels' bounds: the last position has
a segment of its own, so ``flow[b, l, h, that segment, :]`` is the readout's ``mass[b, l, h, :]``.  Against transformers' eager
attention on the same weights in fp32 on the CPU, summed by (seg[i], seg[j]): the relative L2 of ``flow`` is at most 1.25 x that of
the same transformers model run in bf16 (the project's standing criterion; both figures are printed).  Then the plugin's keys and
zero padding.

Measured on MI355X (printed by the tests, recorded in README.md): flow vs HF fp32, rel-L2, next to HF bf16 vs HF fp32 — multi-head
1.69e-4 / 2.37e-4 (ratio 0.71), grouped QK-norm 7.12e-4 / 1.19e-3 (0.60); flow[last segment] vs mass at most 0.0014 of the bound.
"""
import pytest
import torch

import attn_segflow_ref as fr
import probe_harness as ph
from gpu_support import DEV, stop_after_a_device_fault  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PROMPT_LENS = ph.PROMPT_LENS
N_SEG = 5                  # four runs and the last position on its own
S_CAP = 64.0               # scale * sum |q| |k| of bf16 unit-scale rows of these decoders stays below it (as tests/test_gpu_attn_segmass.py takes it)


class _Env(ph.Decoder):
    def __init__(self, kv, qk_norm):
        super().__init__(kv, qk_norm, n_layers=2, redraw=False, row_seed=29)
        self.rt = self.runtime(DEV)
        # four runs, one position ignored, as a query row and as a key, and the last position on its own
        self.segments = [ph.four_runs(n, {n // 2: 255, n - 1: N_SEG - 1}) for n in PROMPT_LENS]

    def hf_flow(self, m, dtype):
        """[B, n_layers, n_heads, n_seg, n_seg] float64: transformers' eager attention matrix summed by (seg[i], seg[j])."""
        m, c = m.to(dtype), self.cfg.llama
        out = torch.zeros(len(self.prompts), c.n_layers, c.n_heads, N_SEG, N_SEG, dtype=torch.float64)
        for b, segs in enumerate(self.prompts):
            with torch.no_grad():
                att = m(input_ids=torch.tensor(segs[0])[None], output_attentions=True).attentions
            ids = torch.tensor(self.segments[b])
            oh = torch.zeros(len(ids), N_SEG + 1, dtype=torch.float64)
            oh[torch.arange(len(ids)), ids.clamp(max=N_SEG)] = 1.0
            for l, a in enumerate(att):
                out[b, l] = torch.einsum("ia,hij,jc->hac", oh[:, :N_SEG], a[0].double(), oh[:, :N_SEG])
        return out


@pytest.fixture(scope="module", params=[(None, False), (2, True)], ids=["mha", "gqa-qknorm"])
def env(request):
    return _Env(*request.param)


def test_runtime(env):
    rt, c = env.rt, env.cfg.llama
    plain = rt.prompt_attention(env.prompts, None, env.segments, n_seg=N_SEG)
    assert plain.flow is None and plain.rows is None
    res = rt.prompt_attention(env.prompts, None, env.segments, n_seg=N_SEG, want_flow=True)
    Bn = len(PROMPT_LENS)
    assert res.flow.shape == (Bn, c.n_layers, c.n_heads, N_SEG, N_SEG) and res.flow.dtype == torch.float32 and res.flow.device.type == "cpu"
    assert res.rows.shape == (Bn, N_SEG) and res.rows.dtype == torch.int64
    assert res.rows.tolist() == [[sg.count(g) for g in range(N_SEG)] for sg in env.segments]
    # bit for bit: first logits and mass are the plain call's, first logits are generate's; chunks of two are one chunk
    assert torch.equal(res.first_logits, plain.first_logits) and torch.equal(res.mass, plain.mass)
    gen = rt.generate(env.prompts, None, max_new_tokens=1, suppress_eos=True, want_first_logits=True)
    assert torch.equal(res.first_logits, gen.first_logits)
    with ph.prefill_chunks(rt, 2):
        chunked = rt.prompt_attention(env.prompts, None, env.segments, n_seg=N_SEG, want_flow=True)
    assert torch.equal(chunked.flow, res.flow) and torch.equal(chunked.mass, res.mass) and torch.equal(chunked.first_logits, res.first_logits)
    assert bool((res.flow >= 0).all())
    # the upper triangle of the runs is empty: a query of run a sees no key of a later run; so is everything the last segment sends
    # to itself but one weight, and a query segment's masses and the ignored key's share sum to its rows
    for b, n in enumerate(PROMPT_LENS):
        for a in range(4):
            assert bool((res.flow[b, :, :, a, a + 1:] == 0).all()), (b, a)
        rel = fr.C1 * c.head_dim * fr.U * S_CAP + fr.C2 * (3 * n + 8) * fr.U + fr.SPLIT
        rows = res.rows[b].double()
        total = res.flow[b].double().sum(-1)                               # [L, H, a]; what is missing went to the ignored key
        assert bool((total <= rows * (1 + rel)).all()), b
        assert bool(((res.flow[b, :, :, 0].double().sum(-1) - rows[0]).abs() <= rows[0] * rel).all()), b      # run 0 lies before it
    # the last position's row of flow is the readout's mass, within the two kernels' bounds (S at its cap)
    worst = 0.0
    for b, n in enumerate(PROMPT_LENS):
        f, m = res.flow[b, :, :, N_SEG - 1, :].double(), res.mass[b].double()
        rel = (fr.C1 * c.head_dim * fr.U * S_CAP + fr.C2 * (3 * n + 8) * fr.U + fr.SPLIT) + \
              (fr.C1 * c.head_dim * fr.U * S_CAP + fr.C2 * (2 * n + 8) * fr.U)
        bound = torch.maximum(f, m) * rel + 3 * n * fr.TINY
        worst = max(worst, float(((f - m).abs() / bound.clamp_min(1e-300)).max()))
        assert bool(((f - m).abs() <= bound).all()), b
    print(f"flow[last segment] vs mass kv={c.n_kv_heads} qk_norm={c.qk_norm}: largest |diff| / bound {worst:.4f}")
    # transformers' eager attention on the same weights, fp32 on the CPU; the reference's own rounding: the same model in bf16
    hf = env.hf()
    want32 = env.hf_flow(hf, torch.float32)
    want16 = env.hf_flow(hf, torch.bfloat16)
    own, got = ph.rel(want16, want32), ph.rel(res.flow.double(), want32)
    print(f"flow kv={c.n_kv_heads} qk_norm={c.qk_norm}: rel-L2 vs HF fp32 {got:.3e}; HF bf16 vs HF fp32 {own:.3e}; "
          f"ratio {got / own:.3f} (allowed {ph.PARITY_RATIO})")
    assert got <= ph.PARITY_RATIO * own


def test_runtime_refusals(env):
    """``check_readout``'s refusals hold with ``want_flow`` and come before anything is sized or launched."""
    rt, c = env.rt, env.cfg.llama
    before = rt.ws.nbytes()
    with pytest.raises(ValueError, match="positions"):
        rt.prompt_attention(env.prompts, None, [s[:-1] for s in env.segments], want_flow=True)
    with pytest.raises(ValueError, match="0..255"):
        rt.prompt_attention(env.prompts[:1], None, [[256] * PROMPT_LENS[0]], want_flow=True)
    with pytest.raises(ValueError, match="at most 32"):
        rt.prompt_attention(env.prompts[:1], None, [list(range(33))], want_flow=True)
    with pytest.raises(ValueError, match="max_pos"):
        rt.prompt_attention([[[5] * (c.max_pos + 1)]], None, [[0] * (c.max_pos + 1)], want_flow=True)
    assert rt.ws.nbytes() == before
    if c.group == 1 and not c.qk_norm:
        r8 = env.runtime(DEV, llm_kv_dtype="fp8")
        with pytest.raises(ValueError, match="bf16 KV cache"):
            r8.prompt_attention(env.prompts, None, env.segments, want_flow=True)


def test_plugin():
    model, b = ph.tiny_plugin_batches(2)
    plain = model.prompt_attention(dict(b))
    out = model.prompt_attention(dict(b), flow=True)
    assert set(plain) == {"mass", "pieces", "first_logits"} and set(out) == {"mass", "pieces", "first_logits", "flow", "rows"}
    c = model.cfg.llama
    n_pieces = max(len(p) for p in out["pieces"])
    assert out["flow"].shape == (2, c.n_layers, c.n_heads, n_pieces, n_pieces) and out["rows"].shape == (2, n_pieces)
    assert torch.equal(out["mass"], plain["mass"]) and torch.equal(out["first_logits"], plain["first_logits"])
    n = 1024
    tol = fr.C1 * c.head_dim * fr.U * S_CAP + fr.C2 * (3 * n + 8) * fr.U + fr.SPLIT
    for r, pc in enumerate(out["pieces"]):
        k = len(pc)
        assert bool((out["rows"][r, :k] > 0).all()) and bool((out["rows"][r, k:] == 0).all())
        assert bool((out["flow"][r, :, :, k:, :] == 0).all()) and bool((out["flow"][r, :, :, :, k:] == 0).all())      # exact zeros behind the pieces
        # every position lies in a piece: a piece's masses sum to its positions; pieces follow each other: nothing flows forward
        rows = out["rows"][r].double()
        assert bool(((out["flow"][r].double().sum(-1) - rows).abs() <= rows * tol).all())
        assert bool((torch.triu(out["flow"][r], diagonal=1) == 0).all())

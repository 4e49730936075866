"""`-m gpu`: the opt-in FP8 KV cache of the LLM decoder (include/icl_hip.h, "FP8 KV cache").

The mode is defined as "the bf16 model whose cache entries are replaced by x' = q * 2^e when they are appended", so every check
here is exact: the append kernels' bytes and scales against torch's own e4m3fn rounding, the fp8 decode attention against the
bf16 kernel on a bf16 cache holding x' (bit-identical), and the fp8-KV models against the runtime's own bf16 kernels with every
appended cache row replaced by x' in torch."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

from decoder_support import same_generation, stream_prompts
from fp8_ref import edge_rows, ref_q
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _rows(shape, seed, spread=(-10, 4)):
    """bf16 rows of very different magnitudes (every row its own exponent)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    mag = torch.exp2(torch.randint(spread[0], spread[1], shape[:-1] + (1,), device=DEV, generator=g).float())
    return (torch.randn(shape, device=DEV, generator=g) * mag).to(BF16)


# ---- quantize-append ---------------------------------------------------------------------------------------------------------
def _append_case(D, H, M, T, seed):
    hd = H * D
    qkv = _rows((M, 3, H, D), seed).reshape(M, 3 * hd)
    ed = edge_rows(D).to(DEV)
    qkv.view(M, 3, H, D)[: len(ed) // 2, 1, 0] = ed[::2]
    qkv.view(M, 3, H, D)[: len(ed) // 2, 2, H - 1] = ed[1::2]
    g = torch.Generator().manual_seed(seed)
    seq = torch.randperm(M, generator=g).to(torch.int32).to(DEV)
    pos = torch.randint(0, T, (M,), generator=g).to(torch.int32).to(DEV)
    kq = torch.full((M, H, T, D), 0x55, dtype=torch.uint8, device=DEV)
    vq = kq.clone()
    ks = torch.full((M, H, T), -1.0, device=DEV)
    vs = ks.clone()
    return qkv, seq, pos, kq, vq, ks, vs


def _check_appended(qkv, seq, pos, kq, vq, ks, vs, H, D, k_rows=None):
    M = qkv.shape[0]
    s, p = seq.long(), pos.long()
    h = torch.arange(H, device=DEV)
    for which, (cq, cs) in ((1, (kq, ks)), (2, (vq, vs))):
        rows = qkv.view(M, 3, H, D)[:, which] if which == 2 or k_rows is None else k_rows
        rb, rs, _ = ref_q(rows)
        assert torch.equal(cq[s[:, None], h[None, :], p[:, None]], rb), which
        assert torch.equal(cs[s[:, None], h[None, :], p[:, None]], rs), which
    untouched = torch.ones(kq.shape[:3], dtype=torch.bool, device=DEV)
    untouched[s[:, None], h[None, :], p[:, None]] = False
    assert bool((kq[untouched] == 0x55).all()) and bool((ks[untouched] == -1).all())


# (128, 11) and (64, 22): a ragged last pass of the two-head-rows-per-thread loop.  A pass is 32 head rows at head_dim 128 and 64 at
# head_dim 64: the rotate form's 3 H = 33 / 66 items end in a second pass with one / two rows in slot 0 and slot 1 empty, the
# append form's 2 H = 22 / 44 fill slot 1 of the only pass in part.
DH_CASES = [(64, 4), (128, 2), (128, 32), (128, 11), (64, 22)]


@pytest.mark.parametrize("D,H", DH_CASES)
def test_prefill_append_bytes_and_scales_match_torch(B, D, H):
    qkv, seq, pos, kq, vq, ks, vs = _append_case(D, H, 37, 11, seed=D + H)
    B.kv_append_fp8(qkv, H * D, 2 * H * D, pos, seq, kq, vq, ks, vs, H, D, 11)
    _check_appended(qkv, seq, pos, kq, vq, ks, vs, H, D)


def test_edge_rows_bytes(B):
    """The edge rows through the kernel, spelled out: zero row -> scale 1 and zero bytes, -0 -> 0x80, 448 * 2^e -> 0x7e."""
    D, H = 64, 1
    ed = edge_rows(D).to(DEV)
    qkv = torch.zeros(len(ed), 3 * D, dtype=BF16, device=DEV)
    qkv[:, D:2 * D] = ed
    qkv[:, 2 * D:] = ed
    seq = torch.arange(len(ed), dtype=torch.int32, device=DEV)
    pos = torch.zeros(len(ed), dtype=torch.int32, device=DEV)
    kq = torch.zeros(len(ed), 1, 1, D, dtype=torch.uint8, device=DEV)
    vq, ks, vs = kq.clone(), torch.zeros(len(ed), 1, 1, device=DEV), torch.zeros(len(ed), 1, 1, device=DEV)
    B.kv_append_fp8(qkv, D, 2 * D, pos, seq, kq, vq, ks, vs, H, D, 1)
    assert torch.equal(kq[0].flatten(), torch.zeros(D, dtype=torch.uint8, device=DEV)) and float(ks[0]) == 1.0
    assert int(kq[2, 0, 0, 7]) == 0x7E and float(ks[2]) == 2.0 ** -3
    assert bool((kq[4] == 0x80).all()) and float(ks[4]) == 1.0
    assert float(ks[1]) == 2.0 ** -7                     # 3 <= 448 * 2^-7 = 3.5 < 448 * 2^-8 * 2
    sub = kq[3, 0, 0]
    assert bool(((sub & 0x78) == 0).any()) and bool(((sub & 0x7F) != 0).any())    # subnormal codes were produced
    rb, rs, _ = ref_q(ed)
    assert torch.equal(kq[:, 0, 0], rb) and torch.equal(ks[:, 0, 0], rs) and torch.equal(vq, kq) and torch.equal(vs, ks)


@pytest.mark.parametrize("D,H", DH_CASES)
def test_decode_rope_append_matches_torch_on_the_bf16_rotation(B, D, H):
    """icl_rope_kv_fp8: q rotated exactly as icl_rope_kv_bf16 rotates it, and the cache holds ref_q of the bf16-rotated k / v."""
    qkv, seq, pos, kq, vq, ks, vs = _append_case(D, H, 8, 16, seed=3 * D + H)
    T, hd, M = 16, H * D, 8
    cos, sin = _rope_tables(64, D)
    ref = qkv.clone()
    kc = torch.zeros(M, H, T, D, dtype=BF16, device=DEV)
    vc = kc.clone()
    B.rope_kv(ref, hd, 2 * hd, cos, sin, pos, seq, kc, vc, H, D, T)
    B.rope_kv_fp8(qkv, hd, 2 * hd, cos, sin, pos, seq, kq, vq, ks, vs, H, D, T)
    assert torch.equal(qkv[:, :hd].view(torch.int16), ref[:, :hd].view(torch.int16))
    _check_appended(qkv, seq, pos, kq, vq, ks, vs, H, D, k_rows=ref.view(M, 3, H, D)[:, 1])


def test_append_outside_the_cache_stores_nothing(B):
    """icl_kv_append_fp8 at a position outside [0, max_len) stores nothing (the only form that reads no table at pos): rows at
    positions -1 and max_len next to two rows that are appended, in planes with a slack sequence on either side, so that a
    missing guard shows as a changed sentinel inside the allocation."""
    M, H, D, T, n_seqs = 4, 2, 64, 4, 6
    qkv = _rows((M, 3 * H * D), 41)
    seq = torch.tensor([1, 2, 3, 4], dtype=torch.int32, device=DEV)
    pos = torch.tensor([-1, T, 0, 3], dtype=torch.int32, device=DEV)
    kq = torch.full((n_seqs, H, T, D), 0x55, dtype=torch.uint8, device=DEV)
    vq = kq.clone()
    ks = torch.full((n_seqs, H, T), -1.0, device=DEV)
    vs = ks.clone()
    B.kv_append_fp8(qkv, H * D, 2 * H * D, pos, seq, kq, vq, ks, vs, H, D, T)
    written = torch.zeros(n_seqs, H, T, dtype=torch.bool, device=DEV)
    for which, cq, cs in ((1, kq, ks), (2, vq, vs)):
        rb, rs, _ = ref_q(qkv.view(M, 3, H, D)[:, which])
        for m in (2, 3):
            s, p = int(seq[m]), int(pos[m])
            assert torch.equal(cq[s, :, p], rb[m]) and torch.equal(cs[s, :, p], rs[m]), (which, m)
            written[s, :, p] = True
        assert bool((cq[~written] == 0x55).all()) and bool((cs[~written] == -1).all()), which
    assert int(written.sum()) == 2 * H


def test_non_finite_rows_become_nan_and_stay_local(B):
    D, H, M, T = 128, 4, 6, 8
    qkv, seq, pos, kq, vq, ks, vs = _append_case(D, H, M, T, seed=5)
    qkv.view(M, 3, H, D)[0, 1, 2, 17] = float("nan")
    qkv.view(M, 3, H, D)[1, 2, 0, 3] = float("inf")
    qkv.view(M, 3, H, D)[2, 1, 1, 0] = float("-inf")
    B.kv_append_fp8(qkv, H * D, 2 * H * D, pos, seq, kq, vq, ks, vs, H, D, T)
    s, p = seq.long(), pos.long()
    for m, cq, cs, h in ((0, kq, ks, 2), (1, vq, vs, 0), (2, kq, ks, 1)):
        assert bool((cq[s[m], h, p[m]] == 0x7F).all()) and bool(torch.isnan(cs[s[m], h, p[m]]))
    ok = qkv.view(M, 3, H, D).clone()
    ok[0, 1, 2] = ok[1, 2, 0] = ok[2, 1, 1] = 0
    rb, rs, _ = ref_q(ok[:, 1])
    hh = torch.arange(H, device=DEV)
    got, gs = kq[s[:, None], hh[None], p[:, None]], ks[s[:, None], hh[None], p[:, None]]
    mask = torch.ones(M, H, dtype=torch.bool, device=DEV)
    mask[0, 2] = mask[2, 1] = False
    assert torch.equal(got[mask], rb[mask]) and torch.equal(gs[mask], rs[mask])
    # the NaN row reaches the attention output of its own (sequence, head) only
    lens = torch.full((M,), T, dtype=torch.int32, device=DEV)
    kq2 = torch.zeros(M, H, T, D, dtype=torch.uint8, device=DEV)
    ks2 = torch.ones(M, H, T, device=DEV)
    kq2[0, 1, 3] = 0x7F
    ks2[0, 1, 3] = float("nan")
    q = _rows((M, H * D), 9)
    out = torch.empty(M, H * D, dtype=BF16, device=DEV)
    B.attn_decode_fp8(q, kq2, kq2, ks2, ks2, out, lens, H, D, T, D ** -0.5)
    bad = torch.isnan(out.float()).view(M, H, D).all(-1)
    expect = torch.zeros(M, H, dtype=torch.bool, device=DEV)
    expect[0, 1] = True
    assert torch.equal(bad, expect)


# ---- decode attention -------------------------------------------------------------------------------------------------------
def _rope_tables(max_pos, D, theta=10000.0):
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    f = torch.arange(max_pos, dtype=torch.float64)[:, None] * inv[None]
    return f.cos().float().to(DEV).contiguous(), f.sin().float().to(DEV).contiguous()


def _cache(n, H, T, D, seed):
    """An fp8 cache of random rows (bytes / scales written by torch) and the bf16 cache holding its x'."""
    x = _rows((2, n, H, T, D), seed)
    q, s, xp = ref_q(x)
    return q[0].contiguous(), q[1].contiguous(), s[0].contiguous(), s[1].contiguous(), xp[0].contiguous(), xp[1].contiguous()


def _lens(n, T, seed):
    base = [1, 5, 385, 384, 2, 7, 100]
    g = np.random.default_rng(seed)
    ls = [base[i] if i < len(base) else int(g.integers(1, T + 1)) for i in range(n)]
    return [min(v, T) for v in ls]


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


# (n_seqs, n_heads): 1 / 7 sequences and 256 x 4 run the "few" unroll (n_seqs * n_heads <= 1024), 256 x 8 the full-chip one
GRID = [(1, 4), (7, 4), (256, 4), (256, 8)]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("n,H", GRID)
def test_attn_decode_fp8_is_bit_identical_to_bf16_on_x_prime(B, D, n, H):
    """Bit for bit against the bf16 kernel with the fp8 kernel's 16-element lane mapping (icl_attn_decode_bf16_epl16) on a bf16
    cache of x'; within 1e-3 (relative L2) of the production 8-element kernel, whose score partial sums run in another order."""
    T = 392
    kq, vq, ks, vs, kx, vx = _cache(n, H, T, D, seed=n * 31 + H + D)
    lens = torch.tensor(_lens(n, T, n), dtype=torch.int32, device=DEV)
    q = _rows((n, H * D), 11, spread=(-2, 2))
    o8 = torch.empty(n, H * D, dtype=BF16, device=DEV)
    ob = torch.empty_like(o8)
    B.attn_decode_fp8(q, kq, vq, ks, vs, o8, lens, H, D, T, D ** -0.5)
    B.attn_decode_bf16_epl16(q, kx, vx, ob, lens, H, D, T, D ** -0.5)
    assert torch.equal(o8.view(torch.int16), ob.view(torch.int16))
    assert bool(torch.isfinite(o8.float()).all())
    op = torch.empty_like(o8)
    B.attn_decode(q, kx, vx, op, lens, H, D, T, D ** -0.5)
    assert _rel(o8, op) <= 1e-3


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("n,H", GRID)
def test_fused_rope_attn_decode_fp8_serves_the_rounded_row(B, D, n, H):
    """icl_attn_decode_rope_fp8 against the bf16 kernels: rope_kv on a bf16 cache holding x', the appended rows then replaced by
    x' in torch, the same-mapping bf16 attention over the cache rows the seq_ids select.  Output and appended bytes bit for bit."""
    T, hd = 392, H * D
    kq, vq, ks, vs, kx, vx = _cache(n, H, T, D, seed=n * 7 + H + D)
    lens_l = _lens(n, T, n + 1)
    lens = torch.tensor(lens_l, dtype=torch.int32, device=DEV)
    pos = lens - 1
    sid = torch.from_numpy(np.random.default_rng(n).permutation(n).astype(np.int32)).to(DEV)      # seq_ids remapping
    qkv = _rows((n, 3 * hd), 13, spread=(-3, 3))
    cos, sin = _rope_tables(T, D)
    kq0, ks0 = kq.clone(), ks.clone()
    o8 = torch.empty(n, hd, dtype=BF16, device=DEV)
    B.attn_decode_rope_fp8(qkv, hd, 2 * hd, cos, sin, pos, sid, kq, vq, ks, vs, o8, lens, H, D, T, D ** -0.5)
    ref = qkv.clone()
    B.rope_kv(ref, hd, 2 * hd, cos, sin, pos, sid, kx, vx, H, D, T)
    s, p, h = sid.long(), pos.long(), torch.arange(H, device=DEV)
    for c in (kx, vx):
        c[s[:, None], h[None], p[:, None]] = ref_q(c[s[:, None], h[None], p[:, None]])[2]
    ob = torch.empty_like(o8)
    B.attn_decode_bf16_epl16(ref[:, :hd], kx[s].contiguous(), vx[s].contiguous(), ob, lens, H, D, T, D ** -0.5)
    assert torch.equal(o8.view(torch.int16), ob.view(torch.int16))
    op = torch.empty_like(o8)
    B.attn_decode(ref[:, :hd], kx[s].contiguous(), vx[s].contiguous(), op, lens, H, D, T, D ** -0.5)
    assert _rel(o8, op) <= 1e-3
    kb, kscale, _ = ref_q(ref.view(n, 3, H, D)[:, 1])
    assert torch.equal(kq[s[:, None], h[None], p[:, None]], kb) and torch.equal(ks[s[:, None], h[None], p[:, None]], kscale)
    vb, vscale, _ = ref_q(qkv.view(n, 3, H, D)[:, 2])
    assert torch.equal(vq[s[:, None], h[None], p[:, None]], vb) and torch.equal(vs[s[:, None], h[None], p[:, None]], vscale)
    kq0[s[:, None], h[None], p[:, None]] = kb
    ks0[s[:, None], h[None], p[:, None]] = kscale
    assert torch.equal(kq, kq0) and torch.equal(ks, ks0)                         # nothing else of the cache was written


def test_kv_copy_spans_fp8_moves_bytes_and_scales(B):
    L, n, H, T, D = 3, 5, 2, 20, 128
    kq = torch.randint(0, 255, (L, n, H, T, D), dtype=torch.uint8, device=DEV)
    ks = torch.randn(L, n, H, T, device=DEV)
    tmp = torch.zeros(L, n, H, 6, D, dtype=torch.uint8, device=DEV)
    tks = torch.zeros(L, n, H, 6, device=DEV)
    src = torch.tensor([4, 0, 2, 2, 1], dtype=torch.int32, device=DEV)
    t0 = torch.tensor([3, 9, 0, 14, 7], dtype=torch.int32, device=DEV)
    B.kv_copy_spans(kq, tmp, n, src_seq=src, src_t0=t0, n_fixed=6, src_scale=ks, dst_scale=tks)
    for r in range(n):
        a, b = int(src[r]), int(t0[r])
        assert torch.equal(tmp[:, r], kq[:, a, :, b:b + 6]) and torch.equal(tks[:, r], ks[:, a, :, b:b + 6])
    view = kq[:, 1:4]                                     # a rows() view: strided sequences
    vs = ks[:, 1:4]
    B.kv_copy_spans(tmp, view, 3, dst_t0=t0, n_fixed=4, src_scale=tks, dst_scale=vs)
    for r in range(3):
        b = int(t0[r])
        assert torch.equal(kq[:, 1 + r, :, b:b + 4], tmp[:, r, :, :4]) and torch.equal(ks[:, 1 + r, :, b:b + 4], tks[:, r, :, :4])


# ---- model level --------------------------------------------------------------------------------------------------------------
def _runtime(kind, kv, wdt="bf16"):
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import QwenAudioCfg, SalmonnCfg
    if kind == "salmonn":
        from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime as R
        cfg = SalmonnCfg.tiny(use_beats=True, lora=True)
        sd = synth.salmonn_state(cfg, seed=0, jitter=True)
        lm = cfg.llama
    else:
        from icl_speech_text_llm_amd.runtime.qwen import QwenAudioRuntime as R
        cfg = QwenAudioCfg.tiny(lora=True)
        sd = synth.qwen_audio_state(cfg, seed=0)
        lm = cfg.llm
    return R(cfg, dict(sd), device=DEV, llm_weight_dtype=wdt, llm_kv_dtype=kv), lm


@contextlib.contextmanager
def xprime_reference(rt):
    """The bf16 runtime as the reference of the fp8-KV model: eager decode (no graph), RoPE + append in the stand-alone
    rope_kv at every batch size, every row appended to the cache replaced by x' in torch — after each rope_kv call, and after
    each prefill (whose attention has used the unrounded k / v by then) — and the decode attention with the fp8 kernel's lane
    mapping (attn_decode_bf16_epl16)."""
    import icl_speech_text_llm_amd.runtime.binding as B
    rope_kv, prefill, attn_decode = B.rope_kv, rt.llama.prefill, B.attn_decode

    def rope_kv_xp(qkv, k_off, v_off, cos, sin, pos, seq_ids, kc, vc, n_heads, head_dim, max_len, M=None):
        rope_kv(qkv, k_off, v_off, cos, sin, pos, seq_ids, kc, vc, n_heads, head_dim, max_len, M=M)
        if kc is not None:
            m = qkv.shape[0] if M is None else M
            s, p, h = seq_ids[:m].long(), pos[:m].long(), torch.arange(n_heads, device=kc.device)
            for c in (kc, vc):
                c[s[:, None], h[None], p[:, None]] = ref_q(c[s[:, None], h[None], p[:, None]])[2]

    def prefill_xp(ws, h, seq_lens, cache=None, **kw):
        out = prefill(ws, h, seq_lens, cache, **kw)
        if cache is not None:
            for b, n in enumerate(seq_lens):
                for c in (cache.k, cache.v):
                    c[:, b, :, :n] = ref_q(c[:, b, :, :n])[2]
        return out

    assert rt.kv_dtype == "bf16"
    B.rope_kv, rt.llama.prefill, B.attn_decode = rope_kv_xp, prefill_xp, B.attn_decode_bf16_epl16
    rt.use_graphs, rt.llama.fuse_decode_rope = False, False
    try:
        yield rt
    finally:
        B.rope_kv, B.attn_decode = rope_kv, attn_decode
        del rt.llama.prefill, rt.use_graphs, rt.llama.fuse_decode_rope


@pytest.fixture(scope="module", params=[("salmonn", "bf16"), ("qwen2", "bf16"), ("salmonn", "fp8"), ("qwen2", "fp8")],
                ids=lambda p: f"{p[0]}-w{p[1]}")
def pair(request):
    """(fp8-KV runtime, bf16-KV runtime of the same weights and weight mode, LLM config)."""
    kind, wdt = request.param
    r8, lm = _runtime(kind, "fp8", wdt)
    rb, _ = _runtime(kind, "bf16", wdt)
    return r8, rb, lm


LENS = [[37], [33, 90, 61, 12, 5, 70, 44, 21], [9 + 7 * i for i in range(16)]]


@pytest.mark.parametrize("lens", LENS, ids=["b1", "b8", "b16"])
def test_first_step_logits_are_bit_identical_to_bf16_mode(pair, lens):
    r8, rb, lm = pair
    prompts = stream_prompts(lm.vocab, lens, seed=len(lens))
    kw = dict(max_new_tokens=1, suppress_eos=True, want_first_logits=True)
    assert torch.equal(r8.generate(prompts, None, **kw).first_logits, rb.generate(prompts, None, **kw).first_logits)


@pytest.mark.parametrize("lens", LENS, ids=["b1", "b8", "b16"])
def test_greedy_step_logits_match_the_x_prime_reference(pair, lens):
    """<= 8 rows: decode runs icl_rope_kv_fp8 + icl_attn_decode_fp8; 16 rows: the fused icl_attn_decode_rope_fp8 — both against
    the bf16 kernels on x' (the reference always runs the stand-alone rope_kv).  Graph-captured fp8 decode included."""
    r8, rb, lm = pair
    prompts = stream_prompts(lm.vocab, lens, seed=len(lens) + 100)
    kw = dict(max_new_tokens=9, suppress_eos=True, want_first_logits=True, want_step_logits=True)
    a = r8.generate(prompts, None, **kw)
    a2 = r8.generate(prompts, None, **kw)               # the second call replays the captured graph
    with xprime_reference(rb):
        b = rb.generate(prompts, None, **kw)
    plain = rb.generate(prompts, None, **kw)
    same_generation(a, b)
    same_generation(a2, b)
    assert torch.equal(a.step_logits, b.step_logits) and torch.equal(a2.step_logits, b.step_logits)
    assert not torch.equal(a.step_logits, plain.step_logits)          # the cache really was rounded


def test_fused_and_unfused_fp8_decode_agree_and_graph_equals_eager(pair):
    r8, _, lm = pair
    prompts = stream_prompts(lm.vocab, [9 + 5 * i for i in range(12)], seed=5)
    kw = dict(max_new_tokens=6, suppress_eos=True, want_step_logits=True)
    fused = r8.generate(prompts, None, **kw)
    r8.use_graphs, r8.llama.fuse_decode_rope = False, False
    try:
        eager_unfused = r8.generate(prompts, None, **kw)
        r8.llama.fuse_decode_rope = True
        eager_fused = r8.generate(prompts, None, **kw)
    finally:
        del r8.use_graphs, r8.llama.fuse_decode_rope
    for o in (eager_unfused, eager_fused):
        same_generation(fused, o)
        assert torch.equal(fused.step_logits, o.step_logits)


def test_sampled_and_beam_match_the_x_prime_reference(pair):
    r8, rb, lm = pair
    prompts = stream_prompts(lm.vocab, [40, 23], seed=3)

    def sampled(rt):
        gen = torch.Generator(device=DEV).manual_seed(1234)
        return rt.generate(prompts, None, max_new_tokens=8, do_sample=True, temperature=0.8, top_p=0.9, top_k=50, generator=gen,
                           want_first_logits=True, suppress_eos=True)
    r8.use_graphs = False
    try:
        a = sampled(r8)
    finally:
        del r8.use_graphs
    with xprime_reference(rb):
        b = sampled(rb)
    same_generation(a, b)
    kw = dict(max_new_tokens=6, suppress_eos=True, num_beams=4, want_first_logits=True)
    a = r8.generate(prompts, None, **kw)
    with xprime_reference(rb):
        b = rb.generate(prompts, None, **kw)
    same_generation(a, b)


@pytest.mark.parametrize("chunk", [1, 3])
def test_chunked_prefill_gives_the_same_bits(pair, chunk):
    r8, _, lm = pair
    prompts = stream_prompts(lm.vocab, [17, 40, 9, 33, 21, 5, 28], seed=11)
    kw = dict(max_new_tokens=5, suppress_eos=True, want_first_logits=True, want_step_logits=True)
    whole = r8.generate(prompts, None, **kw)
    r8.prefill_chunk = chunk
    try:
        part = r8.generate(prompts, None, **kw)
        beams = r8.generate(prompts[:3], None, max_new_tokens=4, suppress_eos=True, num_beams=4)
    finally:
        del r8.prefill_chunk
    same_generation(whole, part)
    assert torch.equal(whole.step_logits, part.step_logits)
    assert torch.equal(beams.tokens, r8.generate(prompts[:3], None, max_new_tokens=4, suppress_eos=True, num_beams=4).tokens)


# ---- full size ----------------------------------------------------------------------------------------------------------------
def test_full_size_fp8_kv_first_logits_and_greedy_ids_match_bf16():
    """Llama-2-7B dims on the decisive-margin weights (bench.margin_parity's set): first-step logits equal bf16 mode bit for bit
    (prefill attends to unrounded k / v), and the 10 greedy decisions equal the bf16 model's."""
    import bench
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    cfg = SalmonnCfg.llama2_7b()
    msd = synth.salmonn_state(cfg, seed=1, device=DEV, dtype=BF16, parts=("llama",), margin=True)
    rt = SalmonnRuntime(cfg, msd, device=DEV, parts=("llama",), consume=True)
    del msd
    _, ids = bench.synth_utterances(0, 1, cfg.llama.vocab)
    g = torch.Generator(device=DEV).manual_seed(0)
    emb = torch.randn(1, bench.N_AUDIO_TOK, cfg.llama.hidden, device=DEV, generator=g) * 0.02
    out = {}
    for kv in ("bf16", "fp8"):
        rt.kv_dtype = kv
        out[kv] = rt.generate(bench.build_prompts(ids[:1]), emb, max_new_tokens=bench.NEW_TOKENS, suppress_eos=True,
                              want_first_logits=True, want_step_logits=True)
    del rt
    torch.cuda.empty_cache()
    assert torch.equal(out["fp8"].first_logits, out["bf16"].first_logits)
    assert out["fp8"].tokens.shape[1] == bench.NEW_TOKENS
    assert torch.equal(out["fp8"].tokens, out["bf16"].tokens), (out["fp8"].tokens, out["bf16"].tokens)
    assert not torch.equal(out["fp8"].step_logits, out["bf16"].step_logits)


# ---- CLI ----------------------------------------------------------------------------------------------------------------------
def test_cli_fp8_kv_writes_the_same_files_as_the_x_prime_reference(tmp_path, monkeypatch):
    from icl_speech_text_llm_amd.inference.inference import main
    from icl_speech_text_llm_amd.runtime import engines
    from icl_speech_text_llm_amd.runtime.salmonn import CausalLMRuntimeMixin
    import icl_speech_text_llm_amd.runtime.binding as B
    common = ["--run_name", "t", "--dataset_type", "voxceleb-hvb", "--arch", "tiny", "--synthetic_items", "3", "--batch_size", "1",
              "--num_workers", "0", "--device", "cuda", "--peft_model_path", ""]
    outs = {}

    def run(tag, extra):
        out = tmp_path / tag
        assert main(common + extra + ["--results_dir", str(out)]) == 0
        files = sorted(os.listdir(out))
        outs[tag] = {f: json.load(open(out / f)) for f in files if f.endswith(("_results.json", "_metrics.json"))}
        assert len(outs[tag]) == 2

    run("fp8", ["--llm_kv", "fp8"])
    with monkeypatch.context() as mp:            # the x' reference of xprime_reference, at class level (the CLI builds its runtime)
        rope_kv, prefill = B.rope_kv, engines.LlamaHIP.prefill

        def rope_kv_xp(qkv, k_off, v_off, cos, sin, pos, seq_ids, kc, vc, n_heads, head_dim, max_len, M=None):
            rope_kv(qkv, k_off, v_off, cos, sin, pos, seq_ids, kc, vc, n_heads, head_dim, max_len, M=M)
            if kc is not None:
                m = qkv.shape[0] if M is None else M
                s, p, h = seq_ids[:m].long(), pos[:m].long(), torch.arange(n_heads, device=kc.device)
                for c in (kc, vc):
                    c[s[:, None], h[None], p[:, None]] = ref_q(c[s[:, None], h[None], p[:, None]])[2]

        def prefill_xp(self, ws, h, seq_lens, cache=None, **kw):
            out = prefill(self, ws, h, seq_lens, cache, **kw)
            if cache is not None:
                for b, n in enumerate(seq_lens):
                    for c in (cache.k, cache.v):
                        c[:, b, :, :n] = ref_q(c[:, b, :, :n])[2]
            return out
        mp.setattr(B, "rope_kv", rope_kv_xp)
        mp.setattr(B, "attn_decode", B.attn_decode_bf16_epl16)
        mp.setattr(engines.LlamaHIP, "prefill", prefill_xp)
        mp.setattr(engines.LlamaHIP, "fuse_decode_rope", False)
        mp.setattr(CausalLMRuntimeMixin, "use_graphs", False)
        run("ref", ["--llm_kv", "bf16"])
    res = [v for k, v in outs["fp8"].items() if k.endswith("_results.json")][0]
    assert len(res) == 6
    assert outs["fp8"] == outs["ref"]

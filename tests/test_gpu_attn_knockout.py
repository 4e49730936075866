"""`-m gpu`: attention knockout.  icl_attn_decode_masked_bf16 against the float64 reference of tests/attn_knockout_ref.py with the
derived bound of tests/test_gpu_attention_exact.py (n and S over the visible keys; tests/test_attn_knockout_ref.py shows on the
CPU that it admits an f32 emulation of the stream order and that the assertions here reject six one-mistake mutants on every form),
then ``generate(knockout=...)`` of the runtime against transformers' eager attention under the same 4-D mask, then the plugin.

Every kernel launch covers oracle.attention.DECODE_LENS (22 cache sequences of 1 .. 320 keys) at max_len 320, NaN in the cache rows
and 0xFF in the segment bytes past each length, the query of sequence row_seq[r] in a row row_q[r] != row_seq[r] of a Q buffer that
is a column slice of a wider one, and O pre-filled with a sentinel bit pattern.  "few" = the 22 entries (at most 88 workgroups),
"many" = enough copies of the list, over the same 22 cache sequences, for more than 1024 workgroups (where the unmasked multi-head
launches switch their unroll; the masked launcher has ONE instantiation per form, so that a row's bits do not depend on the grid).
Which test reaches which instantiation (attn_decode_kernel<D, UNR, false, false, 8, G, true>):
  [D64-H3|4, few|many]      <64, 8, .., 1, true>
  [D128-H3|4, few|many]     <128, 8, .., 1, true>
  [D128-H4|8|14|16-kv2]     <128, 8, .., 2, true>, <128, 4, .., 4 | 7 | 8, true>
Tests (a) - (g) of a form: test_bound (a), test_count_probe (b), test_blocked_peak_probe (c), test_all_masks_zero (d),
test_unlisted_rows_untouched (e), test_batch_invariance (f), test_binding_refuses_what_the_entry_point_refuses (g).

Runtime (the harness of tests/probe_harness.py): 2-layer decoders of hidden 512 (multi-head with the trimmed last layer, grouped
4/2, grouped 4/2 QK-norm), five ragged prompts, one with a speech segment, weights in the style of tests/golden/e2e_weights.py
(layer projections small next to the embeddings and the LM head).  Per step: rel-L2 of the logits against the same transformers
model in fp32 on the CPU, on prompt + generated tokens under the 4-D mask of the knockout (rows >= len - 1, blocked columns at -inf, swapped in
per decoder layer by a forward pre-hook); allowed: 1.25 x the rel-L2 of that model in bf16 against itself in fp32 under the same mask
(the project's ratio criterion).  Both figures are printed.

Measured on MI355X (printed by the tests, recorded in README.md): largest err / bound — random data 0.492 (head_dim 64), 0.484
(128), 0.486 (grouped); offset data 0.296, 0.218, 0.228; blocked-peak probe 0.440, 0.360, 0.365; every mask 0: 0.490, 0.484, 0.486
and at most 1 bf16 ulp from the unmasked kernels (D64-H3: 99.98 % of the elements bit-equal, every other form all).  Logits against
HF fp32 next to HF bf16 against HF fp32, rel-L2, largest ratio of the four steps: multi-head 0.47 (all layers) / 0.46 (window
(1, 2)), grouped 0.45 / 0.47, grouped QK-norm 0.48 / 0.44.
"""
from functools import lru_cache

import pytest
import torch

import attn_knockout_ref as kr
import probe_harness as ph
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)
from oracle import attention as oa

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FA5                   # a NaN bit pattern no kernel writes (int16 view of bf16)
LENS = list(kr.LENS)
SIZES = ("few", "many")


# ------------------------------------------------------------------------------------------------------------------
# the kernel
# ------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _layout():
    seg = kr.make_seg()
    row_seq, row_q = kr.row_list(len(LENS))
    return seg, row_seq, row_q


@lru_cache(maxsize=None)
def _data(kind, form):
    seg, row_seq, row_q = _layout()
    q, kc, vc = kr.data(kind, form)
    return kr.place_q(q, row_seq, row_q), kc, vc


@lru_cache(maxsize=None)
def _blocked(kind, form):
    """The blocked sets of a kind of data: ragged random sets; for "peak" the segment of each (entry, head)'s dominant key; for
    "zero" none."""
    seg, row_seq, row_q = _layout()
    D, H, _ = form
    if kind == "zero":
        return torch.zeros(len(row_seq), H, dtype=torch.int64)
    if kind == "peak":
        qb, kc, vc = _data("peak", form)
        bl, n_blocked = kr.peak_blocked(seg, LENS, row_seq, kr.unmasked_reference(qb, kc, vc, LENS, row_seq, row_q, form, D ** -0.5))
        assert n_blocked > len(row_seq) * H // 2
        return bl
    return kr.blocked_sets(seg, LENS, row_seq, H)


@lru_cache(maxsize=None)
def _ref(kind, form, mask_kind=None):
    """The float64 reference, one row per entry of the 22-entry list: computed once per (data, form, masks) and left unchanged."""
    seg, row_seq, row_q = _layout()
    qb, kc, vc = _data(kind, form)
    return kr.reference(qb, kc, vc, LENS, seg, _blocked(mask_kind or kind, form), row_seq, row_q, form, form[0] ** -0.5)


def _launch(B, form, qbuf, kc, vc, blocked, row_seq, row_q, *, n_q=None, seg=None, lens=LENS):
    """One launch on device copies.  Returns the whole O buffer on the CPU, [n_q, H, D] bf16, sentinel where nothing was written;
    asserts that nothing outside O's columns was touched."""
    D, H, Hkv = form
    hd, n_q = H * D, qbuf.shape[0] if n_q is None else n_q
    seg = _layout()[0] if seg is None else seg
    qw = torch.full((n_q, hd + 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    qw[:qbuf.shape[0], 32:32 + hd] = qbuf.to(DEV)
    ow = torch.full((n_q, hd + 24), 0, dtype=torch.int16, device=DEV).fill_(SENTINEL).view(torch.bfloat16)
    out = ow[:, 8:8 + hd]
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    B.attn_decode_masked(qw[:, 32:32 + hd], kc.to(DEV), vc.to(DEV), out, i32(lens), seg.to(DEV), kr.as_u32_bits(blocked).to(DEV),
                         i32(row_seq), i32(row_q), H, D, kc.shape[2], D ** -0.5, n_kv_heads=Hkv)
    torch.cuda.synchronize()
    raw = ow.view(torch.int16)
    assert bool((raw[:, :8] == SENTINEL).all()) and bool((raw[:, 8 + hd:] == SENTINEL).all()), "wrote outside O"
    return out.cpu().reshape(n_q, H, D)


def _sized(form, size, blocked):
    """(row_seq, row_q, blocked, n_q, reps) of a launch: the 22-entry list, or ``many_reps`` copies of it over the same cache
    sequences, copy c's queries in rows 22 c .. 22 c + 21."""
    _, row_seq, row_q = _layout()
    reps = 1 if size == "few" else kr.many_reps(form[2])
    n = len(row_seq)
    assert (n * reps * form[2] <= 1024) == (size == "few")
    return (row_seq * reps, [c * n + r for c in range(reps) for r in row_q], blocked.repeat(reps, 1), n * reps, reps)


def _run(B, form, size, kind, mask_kind=None):
    """The output rows of the list entries (copy 0), in list order, [22, H, D]; every copy of "many" must hold the same bits."""
    qb, kc, vc = _data(kind, form)
    row_seq, row_q, blocked, n_q, reps = _sized(form, size, _blocked(mask_kind or kind, form))
    out = _launch(B, form, qb.repeat(reps, 1), kc, vc, blocked, row_seq, row_q, n_q=n_q)
    n = len(LENS)
    rows = out[torch.tensor(row_q[:n])]
    for c in range(1, reps):
        assert torch.equal(out[torch.tensor(row_q[c * n:(c + 1) * n])].view(torch.int16), rows.view(torch.int16)), f"copy {c} of the list"
    return rows


def _ulps(a, b):
    """bf16-ulp distance per element (ordered integer codes)."""
    code = lambda x: (lambda i: torch.where(i < 0, -(i & 0x7FFF), i))(x.contiguous().view(torch.int16).int())
    return (code(a) - code(b)).abs()


FORM_SIZE = [pytest.param(f, s, id=f"{kr.form_id(f)}-{s}") for f in kr.FORMS for s in SIZES]


@pytest.mark.parametrize("form,size", FORM_SIZE)
def test_bound(B, form, size):
    """(a) random and offset data, ragged blocked sets: the decode bound, n and S over the visible keys."""
    for kind in ("normal", "offset"):
        worst = oa.assert_bound(_run(B, form, size, kind), _ref(kind, form), form[0], oa.R_P["decode"],
                                f"attn_decode_masked {kr.form_id(form)} {size} {kind}")
        print(f"err/bound attn_decode_masked {kr.form_id(form)} {size} {kind}: {worst:.3f}")


@pytest.mark.parametrize("form,size", FORM_SIZE)
def test_count_probe(B, form, size):
    """(b) q = 0, one-hot V rows: every column is (visible keys feeding it) / (visible keys), one key off moves it."""
    oa.assert_count(_run(B, form, size, "count"), _ref("count", form), f"attn_decode_masked {kr.form_id(form)} {size} count probe")


@pytest.mark.parametrize("form,size", FORM_SIZE)
def test_blocked_peak_probe(B, form, size):
    """(c) the segment of each (entry, head)'s dominant key is blocked: the output is the reference's that lacks it (a kernel that
    ignores the mask returns the dominant key's V row, O(1) away: tests/test_attn_knockout_ref.py)."""
    worst = oa.assert_bound(_run(B, form, size, "peak"), _ref("peak", form), form[0], oa.R_P["decode"],
                            f"attn_decode_masked {kr.form_id(form)} {size} blocked peak")
    print(f"err/bound attn_decode_masked {kr.form_id(form)} {size} blocked peak: {worst:.3f}")


@pytest.mark.parametrize("form,size", FORM_SIZE)
def test_all_masks_zero(B, form, size):
    """(d) every mask 0: inside the same bound of oracle.attention.decode_ref (grouped: on the per-group expanded cache); prints
    the largest bf16-ulp distance to the unmasked kernel (decode-order summation: within rounding, not bit-equal by contract)."""
    D, H, Hkv = form
    _, row_seq, row_q = _layout()
    qb, kc, vc = _data("normal", form)
    got = _run(B, form, size, "normal", "zero")
    q_seq = torch.empty_like(qb)
    q_seq[torch.tensor(row_seq)] = qb[torch.tensor(row_q)]                       # sequence s's query in row s
    kx, vx = (x.repeat_interleave(H // Hkv, dim=1) for x in (kc, vc))
    R = oa.decode_ref(q_seq, kx, vx, LENS, H, D, D ** -0.5).rows(torch.tensor(row_seq))
    worst = oa.assert_bound(got, R, D, oa.R_P["decode"], f"attn_decode_masked {kr.form_id(form)} {size} all masks zero")
    plain = torch.full((len(LENS), H * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    lens_t = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    if Hkv == H:
        B.attn_decode(q_seq.to(DEV), kc.to(DEV), vc.to(DEV), plain, lens_t, H, D, kc.shape[2], D ** -0.5)
    else:
        B.attn_decode_gqa(q_seq.to(DEV), kc.to(DEV), vc.to(DEV), plain, lens_t, H, Hkv, D, kc.shape[2], D ** -0.5)
    torch.cuda.synchronize()
    d = _ulps(got, plain.cpu().view(len(LENS), H, D)[torch.tensor(row_seq)])
    print(f"attn_decode_masked {kr.form_id(form)} {size} all masks zero: err/bound {worst:.3f}; largest distance to the unmasked "
          f"kernel {int(d.max())} bf16 ulp, {float((d == 0).float().mean()):.4%} of the elements bit-equal")


@pytest.mark.parametrize("form", kr.FORMS, ids=kr.form_id)
def test_unlisted_rows_untouched(B, form):
    """(e) every other entry listed, in a permuted order, row_q != row_seq: unlisted rows of O hold the sentinel bit for bit, listed
    rows the bits of the full list's launch."""
    _, row_seq, row_q = _layout()
    qb, kc, vc = _data("normal", form)
    bl = _blocked("normal", form)
    full = _launch(B, form, qb, kc, vc, bl, row_seq, row_q)
    pick = [r for r in range(len(row_seq)) if r % 2 == 0][::-1]
    pick = pick[3:] + pick[:3]
    part = _launch(B, form, qb, kc, vc, bl[torch.tensor(pick)], [row_seq[r] for r in pick], [row_q[r] for r in pick])
    listed = torch.zeros(len(row_q), dtype=torch.bool)
    listed[torch.tensor([row_q[r] for r in pick])] = True
    raw = part.view(torch.int16)
    assert bool((raw[~listed] == SENTINEL).all()), "an unlisted row of O was written"
    assert torch.equal(raw[listed], full.view(torch.int16)[listed]), "a listed row differs from the full list's launch"
    assert not bool((full.view(torch.int16) == SENTINEL).any())


@pytest.mark.parametrize("form", kr.FORMS, ids=kr.form_id)
def test_batch_invariance(B, form):
    """(f) a listed row's bits alone, in the 22-entry list, in the reversed list and in the many-copies launch (more than 1024
    workgroups) are the same."""
    _, row_seq, row_q = _layout()
    qb, kc, vc = _data("normal", form)
    bl = _blocked("normal", form)
    full = _launch(B, form, qb, kc, vc, bl, row_seq, row_q).view(torch.int16)
    rev = _launch(B, form, qb, kc, vc, bl.flip(0), row_seq[::-1], row_q[::-1]).view(torch.int16)
    assert torch.equal(rev, full), "the reversed list gives other bits"
    many = _run(B, form, "many", "normal").view(torch.int16)
    assert torch.equal(many, full[torch.tensor(row_q)]), "the many-copies launch gives other bits"
    for r in range(len(row_seq)):
        one = _launch(B, form, qb, kc, vc, bl[r:r + 1], row_seq[r:r + 1], row_q[r:r + 1]).view(torch.int16)
        assert torch.equal(one[row_q[r]], full[row_q[r]]), f"entry {r} (sequence {row_seq[r]}, {LENS[row_seq[r]]} keys) alone != in the list"


def test_no_visible_key_writes_zeros(B):
    """A (row, head) whose mask leaves no key writes zeros (the L > 0 rule of the bf16 kernel); its neighbours are computed."""
    form = (128, 4, 2)
    D, H, Hkv = form
    lens = [5, 9]
    q, kc, vc = kr.data("normal", form, lens=lens, max_len=16)
    seg = torch.full((2, 16), 0xFF, dtype=torch.uint8)
    seg[0, :5], seg[1, :9] = 3, torch.tensor([0, 0, 1, 1, 1, 2, 2, 40, 40], dtype=torch.uint8)
    bl = torch.tensor([[8, 0, 8, 1], [0, 7, 0, 2]], dtype=torch.int64)          # entry 0: heads 0 and 2 lose every key (id 3)
    out = _launch(B, form, q, kc, vc, bl, [0, 1], [0, 1], seg=seg, lens=lens)
    assert bool((out[0, 0] == 0).all()) and bool((out[0, 2] == 0).all())
    R = kr.reference(q, kc, vc, lens, seg, bl, [0, 1], [0, 1], form, D ** -0.5)
    assert bool((R.n[0] == torch.tensor([0, 5, 0, 5])).all()) and bool((R.n[1] == torch.tensor([9, 2, 9, 6])).all())
    oa.assert_bound(out, R, D, oa.R_P["decode"], "no visible key")


def test_binding_refuses_what_the_entry_point_refuses(B):
    """(g)"""
    D, H, lens = 128, 4, [5, 9]
    q, kc, vc = kr.data("normal", (D, H, H), lens=lens, max_len=16)
    seg = torch.zeros(2, 16, dtype=torch.uint8)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    base = dict(q=q.to(DEV), kc=kc.to(DEV), vc=vc.to(DEV), out=torch.zeros(2, H * D, dtype=torch.bfloat16, device=DEV), lens=i32(lens),
                seg=seg.to(DEV), blocked=torch.zeros(2, H, dtype=torch.int32, device=DEV), row_seq=i32([0, 1]), row_q=i32([1, 0]),
                H=H, D=D, max_len=16, scale=D ** -0.5, Hkv=0)

    def call(**kw):
        a = dict(base, **kw)
        B.attn_decode_masked(a["q"], a["kc"], a["vc"], a["out"], a["lens"], a["seg"], a["blocked"], a["row_seq"], a["row_q"], a["H"],
                             a["D"], a["max_len"], a["scale"], n_kv_heads=a["Hkv"])
    call()                                                                       # the valid call
    wide = torch.zeros(2, H * D + 8, dtype=torch.bfloat16, device=DEV)
    refusals = {
        "n_rows": dict(row_seq=i32([]), row_q=i32([]), blocked=torch.zeros(0, H, dtype=torch.int32, device=DEV)),
        "head_dim": dict(D=96),
        "n_kv_heads": dict(Hkv=3),
        "G at most 8": dict(H=18, Hkv=2, blocked=torch.zeros(2, 18, dtype=torch.int32, device=DEV),
                            q=torch.zeros(2, 18 * D, dtype=torch.bfloat16, device=DEV), out=torch.zeros(2, 18 * D, dtype=torch.bfloat16, device=DEV)),
        "only 128": dict(D=64, H=8, Hkv=4, blocked=torch.zeros(2, 8, dtype=torch.int32, device=DEV)),
        "ld_seg": dict(seg=seg[:, :15].contiguous().to(DEV)),
        "misaligned": dict(q=wide[:, 4:4 + H * D]),
        "ldq": dict(q=torch.zeros(2, H * D - 8, dtype=torch.bfloat16, device=DEV)),
        "ldo": dict(out=torch.zeros(2, H * D - 8, dtype=torch.bfloat16, device=DEV)),
        "scale": dict(scale=float("inf")),
    }
    for word, kw in refusals.items():
        with pytest.raises(B.IclError, match="icl_attn_decode_masked_bf16.*" + word):
            call(**kw)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------
# the runtime
# ------------------------------------------------------------------------------------------------------------------
NEW = ph.NEW
BLOCKED = [[1], [1, 2], [0, 3], [2], [0, 1]]        # per prompt; row 1 blocks its speech segment (1) and the text after it


class _Env(ph.Decoder):
    """The 2-layer decoder of tests/probe_harness.py on the GPU, weights drawn from its ``WEIGHT_SEED``."""

    def __init__(self, kv, qk_norm):
        super().__init__(kv, qk_norm, n_layers=2)
        self.rt = self.runtime(DEV)
        # four runs with one position that can never be blocked and the last one under an id >= 32
        self.segments = [ph.four_runs(n, {n // 2: 255, n - 1: 40}) for n in ph.PROMPT_LENS]
        self.segments[ph.SPEECH_ROW] = ph.speech_row_runs()

    def hf_step_logits(self, m, dtype, tokens, blocked, layers):
        """f64 [NEW, B, V]: transformers, teacher-forced, under the knockout's mask in the decoder layers of the window: rows
        >= len - 1, blocked columns (generated keys are 255) at -inf."""
        def fill_dead(b, n, dead):
            ids = torch.tensor(self.segments[b] + [255] * (NEW - 1))
            dead[n - 1:] |= (torch.isin(ids, torch.tensor(blocked[b], dtype=torch.long)) & (ids < 32))[None]
        out, fired = ph.masked_run(self, m, dtype, tokens, fill_dead, layers)
        assert fired == [layers[1] - layers[0]] * len(self.prompts)
        return out


@pytest.fixture(scope="module", params=[(None, False), (2, False), (2, True)], ids=["mha", "gqa", "gqa-qknorm"])
def env(request):
    return _Env(*request.param)


def _knockout(env, layers=None, heads=None, blocked=BLOCKED):
    return (env.segments, blocked, layers, heads)


@pytest.mark.parametrize("layers", [None, (1, 2)], ids=["all-layers", "window-1-2"])
def test_runtime_against_transformers(env, layers):
    rt, c = env.rt, env.cfg.llama
    sp = env.speech.to(DEV)
    kw = dict(max_new_tokens=NEW, suppress_eos=True, want_first_logits=True, want_step_logits=True)
    res = rt.generate(env.prompts, sp, knockout=_knockout(env, layers), **kw)
    plain = rt.generate(env.prompts, sp, **kw)
    assert res.tokens.shape == (len(env.prompts), NEW) and torch.equal(res.first_logits, res.step_logits[0])
    got = res.step_logits.double().cpu()
    window = (0, c.n_layers) if layers is None else layers
    hf = env.hf()
    want32 = env.hf_step_logits(hf, torch.float32, res.tokens, BLOCKED, window)
    want16 = env.hf_step_logits(hf, torch.bfloat16, res.tokens, BLOCKED, window)
    free32 = env.hf_step_logits(hf, torch.float32, res.tokens, [[]] * len(BLOCKED), window)
    ph.parity_check(got, want32, want16, free32, res.tokens, f"knockout kv={c.n_kv_heads} qk_norm={c.qk_norm} layers={window}",
                    effect_floor=4, min_decisive=res.tokens.numel() // 3, moves="the knockout moves")
    assert not torch.equal(res.step_logits, plain.step_logits)


def test_runtime_mixed_batch_and_empty_sets(env):
    """Rows with an empty blocked set keep the bits of a run without a knockout (logits of every step and tokens), in one chunk
    and in prefill chunks of two; a knockout whose every set is empty is no knockout; heads: only the chosen heads change."""
    rt = env.rt
    sp = env.speech.to(DEV)
    kw = dict(max_new_tokens=NEW, suppress_eos=True, want_first_logits=True, want_step_logits=True)
    plain = rt.generate(env.prompts, sp, **kw)
    mixed_sets = [[], BLOCKED[1], [], [], BLOCKED[4]]
    mixed = rt.generate(env.prompts, sp, knockout=_knockout(env, blocked=mixed_sets), **kw)
    full = rt.generate(env.prompts, sp, knockout=_knockout(env), **kw)
    for b, bl in enumerate(mixed_sets):
        if bl:
            assert torch.equal(mixed.step_logits[:, b], full.step_logits[:, b]) and torch.equal(mixed.tokens[b], full.tokens[b]), b
            assert not torch.equal(mixed.step_logits[:, b], plain.step_logits[:, b]), b
        else:
            assert torch.equal(mixed.step_logits[:, b], plain.step_logits[:, b]) and torch.equal(mixed.tokens[b], plain.tokens[b]), b
            assert torch.equal(mixed.first_logits[b], plain.first_logits[b]), b
    with ph.prefill_chunks(rt, 2):
        chunked = rt.generate(env.prompts, sp, knockout=_knockout(env, blocked=mixed_sets), **kw)
    assert torch.equal(chunked.step_logits, mixed.step_logits) and torch.equal(chunked.tokens, mixed.tokens)
    # twice more: the second call captures the decode graph, the third replays it
    for _ in range(2):
        again = rt.generate(env.prompts, sp, knockout=_knockout(env, blocked=mixed_sets), **kw)
        assert torch.equal(again.step_logits, mixed.step_logits) and torch.equal(again.tokens, mixed.tokens)
    none = rt.generate(env.prompts, sp, knockout=_knockout(env, blocked=[[]] * 5), **kw)
    assert torch.equal(none.step_logits, plain.step_logits) and torch.equal(none.tokens, plain.tokens)
    # an id that cannot be blocked (the last position's 40 is not 8 mod 32) and a segment no position has: nothing effectively
    # blocked, the rows go through the decode-order summation — within rounding of the untouched run, not bit-equal to it
    near = rt.generate(env.prompts, sp, knockout=_knockout(env, blocked=[[8], [8], [8], [8], [8]]), **kw)
    d = float((near.step_logits - plain.step_logits).norm() / plain.step_logits.norm())
    print(f"listed rows with nothing effectively blocked: rel-L2 of the step logits to the untouched run {d:.3e}")
    assert torch.equal(near.tokens, plain.tokens)
    heads = rt.generate(env.prompts, sp, knockout=_knockout(env, heads=[1, 3]), **kw)
    assert not torch.equal(heads.step_logits, full.step_logits) and not torch.equal(heads.step_logits, plain.step_logits)


def test_runtime_other_tails(env):
    """Label-constrained decoding under a knockout returns complete labels and their log-probabilities; sampling runs and is
    reproducible for a seed."""
    from icl_speech_text_llm_amd.runtime.constraints import LabelAutomaton
    rt, c = env.rt, env.cfg.llama
    sp = env.speech.to(DEV)
    # 0 -10-> 1 -11-> 2, 0 -12-> 2, 2 -eos-> accepting: the labels are "10 11" and "12"
    auto = LabelAutomaton([0, 2, 3, 4], [10, 12, 11, c.eos_id], [1, 2, 2, 2], {}, c.vocab, c.eos_id)
    res = rt.generate(env.prompts, sp, max_new_tokens=NEW, knockout=_knockout(env), constraint=(auto, [0] * 5))
    assert res.token_logprobs is not None and res.token_logprobs.shape == res.tokens.shape
    for b in range(5):
        toks = [t for t in res.tokens[b].tolist() if t not in (c.eos_id, c.pad_id)]
        assert toks in ([10, 11], [12]), (b, res.tokens[b].tolist())
    assert bool(torch.isfinite(res.token_logprobs).all()) and bool((res.token_logprobs <= 0).all())
    draws = [rt.generate(env.prompts, sp, max_new_tokens=NEW, suppress_eos=True, do_sample=True, top_k=5, temperature=0.7,
                         generator=torch.Generator().manual_seed(99), knockout=_knockout(env)).tokens for _ in range(2)]
    assert torch.equal(draws[0], draws[1]) and draws[0].shape == (5, NEW)
    assert bool(((draws[0] >= 0) & (draws[0] < c.vocab)).all())


def test_runtime_refusals(env):
    rt, c = env.rt, env.cfg.llama
    sp = env.speech.to(DEV)
    gen = lambda ko, **kw: rt.generate(env.prompts, sp, max_new_tokens=2, knockout=ko, **kw)
    calls = []
    real = rt.llama.prefill
    rt.llama.prefill = lambda *a, **kw: calls.append(1) or real(*a, **kw)
    try:
        before = rt.ws.nbytes()
        with pytest.raises(ValueError, match="num_beams"):
            gen(_knockout(env), num_beams=2)
        with pytest.raises(ValueError, match="positions"):
            gen(([s[:-1] for s in env.segments], BLOCKED))
        with pytest.raises(ValueError, match="for 5 prompts"):
            gen((env.segments[:-1], BLOCKED[:-1]))
        with pytest.raises(ValueError, match="0..255"):
            gen(([[256] + s[1:] for s in env.segments], BLOCKED))
        with pytest.raises(ValueError, match="0..31"):
            gen(_knockout(env, blocked=[[32], [], [], [], []]))
        for bad in ((0, 3), (1, 1), (2, 1), (-1, 1)):
            with pytest.raises(ValueError, match="layer window"):
                gen(_knockout(env, layers=bad))
        for bad in ([4], [-1], []):
            with pytest.raises(ValueError, match="head indices"):
                gen(_knockout(env, heads=bad))
        with pytest.raises(ValueError, match="row 1.*every position"):
            gen(_knockout(env, blocked=[[1], [0, 1, 2], [], [], []]))
        assert rt.ws.nbytes() == before and not calls                       # nothing was sized, nothing launched
    finally:
        del rt.llama.prefill
    # overlong="drop" hands the surviving rows' entries on
    long_row = [[5] * (c.max_pos - 1)]
    res = rt.generate(env.prompts + [long_row], sp, max_new_tokens=NEW, suppress_eos=True, want_step_logits=True, overlong="drop",
                      knockout=(env.segments + [[0] * (c.max_pos - 1)], BLOCKED + [[]]))
    want = rt.generate(env.prompts, sp, max_new_tokens=NEW, suppress_eos=True, want_step_logits=True, knockout=_knockout(env))
    assert res.dropped == (5,) and torch.equal(res.step_logits[:, :5], want.step_logits) and torch.equal(res.tokens[:5], want.tokens)
    if c.group == 1 and not c.qk_norm:                                       # the FP8 KV cache exists for this form only
        r8 = env.runtime(DEV, llm_kv_dtype="fp8")
        with pytest.raises(ValueError, match="bf16 KV cache"):
            r8.generate(env.prompts, sp, max_new_tokens=2, knockout=_knockout(env))


def test_launch_trace():
    """A knockout whose every set is empty launches what no knockout launches; with one, the trace is the two-launch trace (no fused
    RoPE + attention launch) plus exactly one icl_attn_decode_masked_bf16 per windowed layer, per prefill chunk that lists a row and
    per decode step.  On the meta device (tests/tools/launch_trace.py): nothing runs."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    import launch_trace as lt
    lens = list(lt.GEN_LENS)
    segments = [[j % 3 for j in range(n)] for n in lens]

    def trace(cname, knockout, attrs=None, lens=lens, segments=segments):
        rec = lt.Recorder()
        rt = lt.generate_runtime(cname, "bf16", rec)
        for k, v in (attrs or {}).items():
            setattr(rt, k, v)
        with lt.generate_recording(rec):
            rt.generate(lt.prompts_of(lens), None, max_new_tokens=4, **({} if knockout is None else {"knockout": knockout(segments)}))
        return rec.log

    masked = lambda log: [x for x in log if x.startswith("attn_decode_masked(")]
    for cname in ("tiny_h4", "7b_gqa8_bias", "7b_nolora"):
        n_layers = lt.configs()[cname].n_layers
        plain = trace(cname, None)
        assert trace(cname, lambda s: (s, [[]] * len(lens))) == plain, cname
        for window in (None, (1, 2)):
            n_win = n_layers if window is None else window[1] - window[0]
            for attrs, chunks in (({}, 1), (dict(prefill_chunk=2), 2)):          # rows 0 and 3 listed: chunks [0, 1] and [2, 3] of three
                log = trace(cname, lambda s: (s, [[0], [], [], [1, 2], []], window), attrs)
                assert len(masked(log)) == n_win * (chunks + 3), (cname, window, attrs)
                rest = [x for x in log if not x.startswith("attn_decode_masked(")]
                base = trace(cname, None, attrs)
                kinds = lambda lg: [x.split("(")[0] for x in lg if "(" in x and not x.startswith("torch.")]
                assert kinds(rest) == kinds(base), (cname, window, attrs)
    # many rows (the fused RoPE + attention launch without a knockout): with one, the two-launch form
    big, seg_big = [5] * 12, [[j % 3 for j in range(5)]] * 12
    plain = trace("7b_nolora", None, lens=big, segments=seg_big)
    log = trace("7b_nolora", lambda s: (s, [[0]] + [[]] * 11), lens=big, segments=seg_big)
    names = lambda lg: [x.split("(")[0] for x in lg]
    assert "attn_decode_rope" in names(plain) and "attn_decode_rope" not in names(log)
    assert names(log).count("rope_kv") - names(plain).count("rope_kv") == names(plain).count("attn_decode_rope") == names(log).count("attn_decode") - names(plain).count("attn_decode")


# ------------------------------------------------------------------------------------------------------------------
# the plugin
# ------------------------------------------------------------------------------------------------------------------
def test_plugin():
    model, b = ph.tiny_plugin_batches(2)
    with ph.spy_generate(model) as seen:
        out = model.generate_knockout(dict(b), [("example", 1)])
    assert set(out) == {"texts", "tokens", "first_logits", "pieces"}
    c = model.cfg.llama
    assert len(out["texts"]) == 2 and out["tokens"].shape[0] == 2 and out["first_logits"].shape == (2, c.vocab)
    att = model.prompt_attention(dict(b))
    assert out["pieces"] == att["pieces"]
    segments, blocked, layers, heads = seen["kw"]["knockout"]
    assert layers is None and heads is None
    assert blocked == [[pc.index(("example", 1))] for pc in out["pieces"]]
    for sg, pc in zip(segments, out["pieces"]):                                  # the ids of prompt_attention's pieces
        assert sorted(set(sg)) == list(range(len(pc)))
    plain = model.generate_ids(dict(b), want_first_logits=True)
    assert not torch.equal(out["first_logits"], plain.first_logits)
    per_row = model.generate_knockout(dict(b), [[("example", 1)], []], layers=(0, 1), heads=[0])
    assert torch.equal(per_row["first_logits"][1], plain.first_logits[1]) and not torch.equal(per_row["first_logits"][0], plain.first_logits[0])
    with pytest.raises(ValueError, match="row 0.*no piece"):
        model.generate_knockout(dict(b), [("example", 7)])
    assert torch.equal(model.generate_ids(dict(b), want_first_logits=True).first_logits, plain.first_logits)      # generate_output's path is untouched

"""CPU: the prompt-attention readout without a GPU.  (1) The bound of tests/attn_segmass_ref.py is usable and sharp: an f32 numpy
emulation of the definition stays inside it on every case tests/test_gpu_attn_segmass.py runs, and every mutant reference (one key
dropped, the last key duplicated, lens off by one, a segment boundary moved by one key, an ignored id counted into segment 0) is
rejected on every case.  (2) The argument checks of icl_attn_segmass_bf16, called with host pointers or NULL: each refusal returns
-1 and names the argument, before any launch.  (3) The plugin's per-position piece ids against interleave_plan."""
import ctypes
import math

import pytest
import torch

import attn_segmass_ref as sr


@pytest.fixture(scope="module")
def data():
    """Per case: the random inputs, their segments and the float64 reference, computed once."""
    out = {}
    for case in sr.CASES:
        D, H, Hkv, n_seg = case
        q, kc = sr.random_case(sr.LENS, H, Hkv, D)
        seg = sr.make_seg(sr.LENS, n_seg)
        out[case] = (q, kc, seg, sr.reference(q, kc, sr.LENS, seg, n_seg, H, Hkv, D, D ** -0.5))
    return out


def test_cases_cover_the_forms():
    assert {c[0] for c in sr.CASES} == {64, 128} and {c[3] for c in sr.CASES} == {1, 2, 32}
    assert {c[1] // c[2] for c in sr.CASES} == {1, 2, 4, 7, 8} and all(D == 128 for D, H, Hkv, _ in sr.CASES if H != Hkv)
    for n_seg in (1, 2, 32):
        seg = sr.make_seg(sr.LENS, n_seg)
        assert bool((seg[:, sr.MAX_LEN - 1] == 0xFF).all())
        used = [set(seg[b, :L].tolist()) for b, L in enumerate(sr.LENS)]
        assert any(any(x >= n_seg for x in u) for u in used), "no ignored id inside a length"
        assert all(any(x < n_seg for x in u) for u in used)
        if n_seg >= 2:
            assert all(1 not in u for u in used) or n_seg == 2        # an empty segment in every row (n_seg 32), in some (n_seg 2)
            assert any(len({x for x in u if x < n_seg}) < n_seg for u in used)


@pytest.mark.parametrize("case", sr.CASES, ids=sr.case_id)
def test_f32_emulation_is_inside_the_bound(data, case):
    D, H, Hkv, n_seg = case
    q, kc, seg, R = data[case]
    mass, probs = sr.emulate_f32(q, kc, sr.LENS, seg, n_seg, H, Hkv, D, D ** -0.5)
    wm, wp = sr.worst(mass, probs, R, D)
    print(f"f32 emulation {sr.case_id(case)}: err/bound mass {wm:.3f}, probs {wp:.3f}")
    assert wm <= 1 and wp <= 1
    assert bool((mass[R.n_g[:, None, :].expand_as(R.mass) == 0] == 0).all())           # an empty segment is exactly 0
    # with ignored ids inside the length the masses sum to the reference's partial sum, not to 1
    assert float((R.mass.sum(-1) - 1).abs().max()) > 1e-3


# every mutant on every case, but for the boundary mutant where there is one segment and so no boundary to move
MUTANT_CASES = [(c, m) for c in sr.CASES for m in sr.MUTANTS if not (m == "move_boundary" and c[3] == 1)]


@pytest.mark.parametrize("case,mutant", MUTANT_CASES, ids=[f"{sr.case_id(c)}-{m}" for c, m in MUTANT_CASES])
def test_mutants_are_rejected(data, case, mutant):
    D, H, Hkv, n_seg = case
    q, kc, seg, R = data[case]
    M = sr.reference(q, kc, sr.LENS, seg, n_seg, H, Hkv, D, D ** -0.5, mutate=mutant)
    wm, wp = sr.worst(M.mass, M.probs, R, D)
    print(f"mutant {mutant} {sr.case_id(case)}: err/bound mass {wm:.3g}, probs {wp:.3g}")
    assert wm > 1, "the mass bound admits the mutant"
    if mutant not in sr.SEG_MUTANTS:
        assert wp > 1, "the probs bound admits the mutant"


def test_probes_meet_their_conditions():
    """The count probe's reference is 1 / n and n_g / n; the peak probe's target segment holds >= 1 - 2^-12 of the mass on the
    reference (never on the kernel), for every head's target: first key, last key, a segment's first and last key."""
    for D, H, Hkv, n_seg in ((64, 4, 4, 2), (128, 3, 3, 32), (128, 16, 2, 32)):
        seg = sr.make_seg(sr.LENS, n_seg)
        q, kc = sr.count_probe(sr.LENS, H, Hkv, D)
        R = sr.reference(q, kc, sr.LENS, seg, n_seg, H, Hkv, D, D ** -0.5)
        want = R.live[:, None, :].double() / R.n[:, None, None]
        assert float((R.probs - want).abs().max()) < 1e-15
        assert float((R.mass - (R.n_g / R.n[:, None])[:, None, :]).abs().max()) < 1e-13
        q, kc, tgt = sr.peak_probe(sr.LENS, H, Hkv, D, seg, n_seg)
        R = sr.reference(q, kc, sr.LENS, seg, n_seg, H, Hkv, D, D ** -0.5)
        kinds = set()
        for b, L in enumerate(sr.LENS):
            t = sr.peak_targets(seg[b], L, n_seg)
            assert t[0] == 0 and t[1] == L - 1
            for h in range(H):
                g = int(seg[b, tgt[b, h]])
                assert float(R.probs[b, h, tgt[b, h]]) >= sr.W_EXACT
                if g < n_seg:
                    assert float(R.mass[b, h, g]) >= sr.W_EXACT
                    kinds.add(h % 4)
        assert kinds == set(range(min(H, 4)))


# ------------------------------------------------------------------------------------------------------------------
# the entry point's argument checks (host pointers: every refusal comes before any launch)
# ------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_and_refuses_bad_arguments():
    import icl_speech_text_llm_amd.runtime.binding as b
    assert "icl_attn_segmass_bf16" in b.EXPORTED_SYMBOLS and b.ABI_VERSION == 6
    lib = b.load_library()
    buf = ctypes.create_string_buffer(4096)                 # 16-byte aligned host memory stands in for every operand
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    good = dict(Q=p, ldq=512, q_rows=None, Kc=p, lens=p, seg=p, ld_seg=64, n_seg=4, mass=p, probs=None, ld_probs=0, n_seqs=1,
                n_heads=4, n_kv_heads=0, head_dim=128, max_len=64, scale=0.1, stream=None)

    def refused(word, **kw):
        a = dict(good, **kw)
        rc = lib.icl_attn_segmass_bf16(*a.values())
        msg = lib.icl_last_error()
        assert rc == -1 and b"icl_attn_segmass_bf16" in msg and word in msg, (kw, rc, msg)

    for name in ("Q", "Kc", "lens", "seg", "mass"):
        refused(name.encode(), **{name: None})
    refused(b"n_seg", n_seg=0)
    refused(b"n_seg", n_seg=33)
    refused(b"head_dim", head_dim=96)
    refused(b"n_kv_heads", n_kv_heads=3)                    # 4 % 3
    refused(b"n_kv_heads", n_heads=18, n_kv_heads=2, ldq=18 * 128)      # G = 9
    refused(b"head_dim", n_heads=4, n_kv_heads=2, head_dim=64)          # G = 2 at head_dim 64
    refused(b"ld_seg", ld_seg=63)
    refused(b"ld_probs", probs=p, ld_probs=63)
    for bad in (math.inf, -math.inf, math.nan):
        refused(b"scale", scale=bad)


# ------------------------------------------------------------------------------------------------------------------
# the plugin's piece ids
# ------------------------------------------------------------------------------------------------------------------
class _Tok:
    """One id per character (an empty part gives no ids), in the call shape CustomSALMONN uses."""

    def __call__(self, text, **_):
        return {"input_ids": torch.tensor([[ord(c) % 200 + 3 for c in text]], dtype=torch.long).reshape(1, -1)}


def _pieces(prompt, embeds, num_examples, example_embeds):
    from icl_speech_text_llm_amd.models.custom_salmon import CustomSALMONN
    m = object.__new__(CustomSALMONN)                       # the prompt logic alone: no weights, no device
    m.__dict__.update(llama_tokenizer=_Tok(), speech_placeholder="<SpeechHere>", device=torch.device("cpu"))
    segs, _, pieces = m._segments_and_pieces(embeds, [prompt], torch.tensor([num_examples]), example_embeds)
    return segs[0], pieces[0], CustomSALMONN.piece_ids(segs[0])


def _check_ids(segs, pieces, ids, plan, empty_text):
    from icl_speech_text_llm_amd.runtime.salmonn import _is_speech
    want = [e for e in plan if not (e[0] == "text" and e[1] in empty_text)]
    assert pieces == want                                                   # the plan's order, empty text parts skipped
    lens = [s[2] if _is_speech(s) else len(s) for s in segs]
    assert ids == [p for p, n in enumerate(lens) for _ in range(n)] and len(ids) == sum(lens)
    for (kind, _), s in zip(pieces, segs):
        assert _is_speech(s) == (kind != "text")


def test_plugin_piece_ids_follow_the_interleave_plan():
    from icl_speech_text_llm_amd.models.custom_salmon import interleave_plan, interleave_plan_sqa
    sp = lambda n: torch.zeros(n, 8)
    # two exemplars; the prompt begins with <Example0>, so text part 0 is empty and gets no id
    segs, pieces, ids = _pieces("<Example0> is A. <Example1> is B. Now <SpeechHere> is", sp(5)[None], 2, [[sp(3), sp(4)]])
    plan = interleave_plan(4, 2, 2, True)
    _check_ids(segs, pieces, ids, plan, empty_text={0})
    assert pieces == [("example", 0), ("text", 1), ("example", 1), ("text", 2), ("speech", 0), ("text", 3)]
    assert ids[:3] == [0, 0, 0] and ids[-3:] == [5, 5, 5] and ids.count(4) == 5 and ids.count(2) == 4
    # zero-shot
    segs, pieces, ids = _pieces("Listen: <SpeechHere> What is it?", sp(6)[None], 0, None)
    _check_ids(segs, pieces, ids, interleave_plan(2, 0, None, True), empty_text=set())
    assert pieces == [("text", 0), ("speech", 0), ("text", 1)] and ids.count(1) == 6
    # SQA: one exemplar (document + question audio), then the query's document and question
    prompt = "D: <Document0> Q: <Question0> A: yes. D: <Document> Q: <Question> A:"
    segs, pieces, ids = _pieces(prompt, (sp(2)[None], sp(3)[None]), 1, [[(sp(4), sp(5))]])
    _check_ids(segs, pieces, ids, interleave_plan_sqa(5, 1, 1, True), empty_text=set())
    assert [k for k, _ in pieces] == ["text", "example_d", "text", "example_q", "text", "speech_d", "text", "speech_q", "text"]
    assert ids.count(1) == 5 and ids.count(3) == 4 and ids.count(5) == 3 and ids.count(7) == 2      # d = [1] of a pair, q = [0]

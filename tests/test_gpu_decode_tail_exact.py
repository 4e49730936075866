"""The two kernels that decide which token is emitted — sample_eos_kernel (csrc/sampling.hip) and beam_step_kernel
(csrc/beam.hip) — against the float64 references of oracle/decode_tail.py, one launch at a time (`-m gpu`; every call goes
through runtime/binding.py).  The bounds are derived in oracle/decode_tail.py, none fitted; tests/test_decode_tail_bounds.py
shows on the CPU, over these very inputs (tests/decode_tail_cases.py), that an f32 emulation in the kernels' order passes
these checks, that a kernel with one mistake does not, and that at most 10 % of the rows / steps of each test are ambiguous.

What is asserted (tests/fp64_bounds.py: check_sampler_row, check_beam_row):
  sampler   the `work` scores bit for bit (two IEEE f32 operations: the library is built without fast-math and hipcc divides
            correctly rounded by default, so no ulp is granted), sentinels in work[V..ldw), in the debug rows past the count, in
            the token buffer and around every per-row output; the kept ids in draw order (exact); count in [keep_lo, keep_hi];
            every kept probability within its bound of the float64 value renormalised over the kernel's own count; a pick
            that the draw justifies; finished / EOS / pad bookkeeping.  Determinate rows (every deciding gap above twice its
            bound): count and pick equal the float64 ones.
  beam      ranges, run_seq = the parent's sequence + the token, run_score within the bound of the float64 score of the
            (parent, token) chosen and that score within the bounds of the rank taken, closed rows untouched; determinate
            steps: parents, tokens, sequences, lengths, flags, unsat equal, fin_score within the bound / length penalty.
Each test prints `err/bound <kernel> <case>: <worst>; ambiguous a/n`; the measured figures are in DESIGN.md.

The overflow rows (more than 1024 tokens at or above the cut) are launched twice and must agree bit for bit; before the
candidate list was rebuilt by rule (strictly greater first, ties by ascending id) they kept whichever tokens the atomics
delivered first, and a listed NaN made every probability NaN (test_sampler_grid at V = 50, top_k = V).
"""
import numpy as np
import pytest
import torch

import decode_tail_cases as dc
import fp64_bounds as fb
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
CAP = 1024


def _guarded(n, fill, dtype):
    """(buffer of n + 2 with `fill` everywhere, its inner view of n)."""
    buf = torch.full((n + 2,), fill, dtype=dtype, device=DEV)
    return buf, buf[1:n + 1]


def _launch_sampler(B, c):
    """One icl_sample_eos launch of case `c`; returns the per-row outputs (numpy) after the sentinel checks that concern the
    launch as a whole."""
    Bn, V, S = c["logits"].shape[0], c["V"], float(c["sentinel"])
    lg = torch.from_numpy(c["logits"]).to(DEV)
    work = torch.full((Bn, c["ldw"]), S, dtype=F32, device=DEV)
    toks = torch.from_numpy(c["tokens"]).to(DEV)
    fin_buf, fin = _guarded(Bn, 77, I32)
    fin.copy_(torch.from_numpy(c["finished"]))
    nxt_buf, nxt = _guarded(Bn, -7, I32)
    cnt_buf, cnt = _guarded(Bn, -9, I32)
    ids = torch.full((Bn, CAP), -1, dtype=I32, device=DEV)
    probs = torch.full((Bn, CAP), S, dtype=F32, device=DEV)
    u = torch.from_numpy(c["u"]).to(DEV)
    B.sample_eos(lg, work, u, c["eos"], c["pad"], fin, toks, c["step"], nxt, temperature=c["temp"], top_k=c["top_k"],
                 top_p=c["top_p"], repetition_penalty=c["pen"], V=V, debug=(ids, probs, cnt))
    torch.cuda.synchronize()
    assert fin_buf[[0, -1]].tolist() == [77, 77] and nxt_buf[[0, -1]].tolist() == [-7, -7] and cnt_buf[[0, -1]].tolist() == [-9, -9]
    assert np.array_equal(lg.cpu().numpy().view(np.uint32), c["logits"].view(np.uint32)), "the launch wrote its input"
    assert np.array_equal(u.cpu().numpy(), c["u"])
    work, toks, fin, nxt, cnt, ids, probs = (t.cpu().numpy() for t in (work, toks, fin, nxt, cnt, ids, probs))
    return [dict(work=work[b], ids=ids[b], probs=probs[b], count=cnt[b], next_id=nxt[b], tokens=toks[b], finished=fin[b])
            for b in range(Bn)]


def _run_sampler(B, cases, tag, twice=False):
    worst, amb, rows = 0.0, 0, 0
    for c in cases:
        outs = _launch_sampler(B, c)
        if twice:
            again = _launch_sampler(B, c)
            for b, (o1, o2) in enumerate(zip(outs, again)):
                for k in ("ids", "probs", "count", "next_id"):
                    assert np.array_equal(np.asarray(o1[k]).view(np.uint32), np.asarray(o2[k]).view(np.uint32)), \
                        f"{c['name']}[{b}]: {k} differs between two identical launches"
        for b, out in enumerate(outs):
            r, a = fb.check_sampler_row(c, b, out, f"{c['name']}[{b}]")
            worst, amb, rows = max(worst, r), amb + int(a), rows + 1
    print(f"err/bound sample_eos {tag}: {worst:.3f}; ambiguous {amb}/{rows}")
    assert amb <= 0.10 * rows, f"{tag}: {amb} of {rows} rows ambiguous"


@pytest.mark.parametrize("V", [1, 50, 255, 256, 257, 1024, 1025, 32001])
def test_sampler_grid(B, V):
    """top_k in {1, 2, 50, 1024, V} x top_p in {1, 0.9, 1e-6}, each as B = 1 / step 0 / dense rows and as B = 5 / step 300
    (n_prev > 256) / ldl = V + 5, ldw = V + 3 with +inf and NaN in the pad columns / penalty 1.3 on a history with duplicates,
    -1, ids >= V, the pad id and hits on negative, positive and zero logits.  The five rows: Gaussian (u = 0), peaked
    (u = nextafter(1, 0)), nearly flat, ties straddling the top-k cut, NaN and -inf logits; one more launch draws on a CDF step."""
    _run_sampler(B, dc.sampler_test_cases(V), f"grid V={V}")


def test_sampler_full_qwen_vocabulary(B):
    _run_sampler(B, [dc.sampler_large_case()], "V=156032")


def test_sampler_bookkeeping(B):
    """Finished rows emit pad, either EOS id finishes a row, the pad id does not."""
    c = dc.sampler_bookkeeping_case()
    outs = _launch_sampler(B, c)
    assert [int(o["next_id"]) for o in outs] == [9, 100, 256, 9, 200, 9]
    assert [int(o["finished"]) for o in outs] == [1, 1, 1, 0, 0, 1]
    _run_sampler(B, [c], "bookkeeping")


def test_sampler_greedy_with_repetition_penalty(B):
    """temperature 1, top_k 1, top_p 1, u 0: the lowest-id arg-max of the penalised row."""
    c = dc.sampler_greedy_penalty_case()
    outs = _launch_sampler(B, c)
    assert [int(o["next_id"]) for o in outs] == [12, 500, 41]
    _run_sampler(B, [c], "greedy+penalty")


def test_sampler_scores_past_expf_overflow(B):
    _run_sampler(B, [dc.sampler_hot_case()], "hot scores")


def test_sampler_candidate_list_overflow(B):
    """More than 1024 tokens at or above the cut: every token strictly above it is listed, then the tied ones by ascending id;
    probabilities are finite, a -inf token has probability 0 and is never picked; two identical launches agree bit for bit."""
    cases = dc.sampler_overflow_cases()
    _run_sampler(B, cases, "overflow", twice=True)
    by = {c["name"]: c for c in cases}
    outs = _launch_sampler(B, by["ten-above-2000-ties-k50"])
    V = 32001
    assert outs[0]["ids"][:10].tolist() == list(range(V - 1, V - 11, -1)) and int(outs[0]["next_id"]) == V - 1
    outs = _launch_sampler(B, by["masked-3-finite-k50"])
    for o in outs:
        assert o["ids"][:3].tolist() == [20000, 31990, 17] and int(o["next_id"]) in (20000, 31990, 17)
        assert bool((o["probs"][3:int(o["count"])] == 0).all())
    assert [int(o["next_id"]) for o in _launch_sampler(B, by["all-equal-k1"])][0] == 0
    assert [int(o["next_id"]) for o in _launch_sampler(B, by["greedy-over-flat"])] == [V - 3] * 3


# ---- beam step -----------------------------------------------------------------------------------------------------------------
_STATE = ("run_score", "run_seq", "fin_score", "fin_seq", "fin_len", "fin_flag", "unsat")


class _Guarded:
    """Allocator for binding.BeamState: every buffer sits between two sentinel words."""

    def __init__(self):
        self.bufs = []

    def __call__(self, name, shape, dt):
        n = int(np.prod(shape))
        fill = -777.0 if dt == F32 else -777
        buf, view = _guarded(n, fill, dt)
        self.bufs.append((name, buf, fill))
        return view.view(*shape)

    def check(self):
        for name, buf, fill in self.bufs:
            assert buf[[0, -1]].tolist() == [fill, fill], f"{name}: written outside the buffer"


def _beam_launch(B, params, logits, state_np):
    """One icl_beam_step launch from `state_np` (numpy dict, [B, ...]); returns the outgoing state + next_ids / parent."""
    Bn, K, T, V = params["B"], params["K"], params["T"], params["V"]
    g = _Guarded()
    st = B.BeamState(g, Bn, K, T, pad_id=0)
    for k in _STATE:
        getattr(st, k).copy_(torch.from_numpy(np.ascontiguousarray(state_np[k])).to(DEV))
    st.next_ids.fill_(-5)
    st.parent.fill_(-5)
    lg = torch.from_numpy(logits).to(DEV)
    B.beam_step(lg, st, params["step"], params["eos"], params["lp"], V=V, repetition_penalty=params["pen"])
    torch.cuda.synchronize()
    g.check()
    assert np.array_equal(lg.cpu().numpy().view(np.uint32), logits.view(np.uint32)), "the launch wrote its input"
    out = {k: getattr(st, k).cpu().numpy() for k in _STATE}
    out["next_ids"] = st.next_ids.cpu().numpy().reshape(Bn, K)
    out["parent"] = st.parent.cpu().numpy().reshape(Bn, K) - np.arange(Bn)[:, None] * K
    return out


def _check_beam_launch(params, logits, old_state, out, tag):
    worst, amb = 0.0, 0
    rpb = params["rows"]
    for b in range(params["B"]):
        old = dc.beam_row_view(old_state, b)
        ref = dc.beam_row_ref(params, logits[b * rpb:(b + 1) * rpb], old)
        row = {k: (v[b] if k != "unsat" else int(v[b])) for k, v in out.items()}
        r, a = fb.check_beam_row(ref, row, old, f"{tag}[{b}]")
        worst, amb = max(worst, r), amb + int(a)
    return worst, amb


def test_beam_single_launches(B):
    """Crafted incoming state, several rows of different state per launch: V == NC ((1,2), (4,8), (2,6) with two EOS ids),
    V in {40, 255, 257, 32001}, K = 8 / T = 64 at steps 0, 1, 62, 63, rows_per_batch 1 and K, ldl > V with +inf behind the
    row, -inf leaving fewer than NC finite continuations, length penalty 0 / 1 / 2 / -1, repetition penalty 1.6 on histories
    with duplicates and the pad id, closed rows, partly filled and full finished slots that are / are not displaced, EOS at
    rank < K and >= K, logits past expf's overflow."""
    worst, amb, rows = 0.0, 0, 0
    for c in dc.beam_single_cases():
        out = _beam_launch(B, c, c["logits"], c["state"])
        w, a = _check_beam_launch(c, c["logits"], c["state"], out, c["name"])
        worst, amb, rows = max(worst, w), amb + a, rows + c["B"]
    print(f"err/bound beam_step single launches: {worst:.3f}; ambiguous {amb}/{rows}")
    assert amb <= 0.10 * rows


@pytest.mark.parametrize("setup", dc.beam_search_setups(), ids=lambda s: s[0])
def test_beam_whole_search_on_the_kernels_own_history(B, setup):
    """Every step is judged from the state the kernel itself left (read back before the launch); the logits follow the
    kernel's parents and tokens."""
    name, Bn, K, V, T, eos, lp, pen, seed = setup
    model = dc.SearchLogits(Bn, K, V, eos, seed)
    state = dc.beam_state(Bn, K, T, V - 1)
    worst, amb, steps = 0.0, 0, 0
    for s in range(T):
        lg = model.logits()
        p = dict(B=Bn, K=K, V=V, T=T, step=s, eos=eos, lp=lp, pen=pen, rows=lg.shape[0] // Bn)
        out = _beam_launch(B, p, lg, state)
        w, a = _check_beam_launch(p, lg, state, out, f"{name} step {s}")
        worst, amb, steps = max(worst, w), amb + a, steps + Bn
        model.advance((out["parent"] + np.arange(Bn)[:, None] * K).reshape(-1), out["next_ids"].reshape(-1))
        state = {k: out[k] for k in _STATE}
    print(f"err/bound beam_step {name}: {worst:.3f}; ambiguous {amb}/{steps}")
    assert amb <= 0.10 * steps

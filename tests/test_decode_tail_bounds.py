"""CPU twin of test_gpu_decode_tail_exact.py (no GPU, no library): the float64 references of oracle/decode_tail.py and the
checkers of tests/fp64_bounds.py, run over every input the GPU module launches (tests/decode_tail_cases.py).

  * the float64 sampler reference reproduces HF's processors (tests/golden/sampling.npz) and agrees with the float32
    restatement oracle.models.sample_filter on the random cases of test_gpu_kernels.py;
  * the float64 beam reference agrees step for step with the float32 BeamBookkeeping on determinate steps of whole searches;
  * a numpy float32 emulation of each kernel's summation order passes the GPU module's checks on every GPU-test input (the
    worst err / bound is printed, and must be below 1), and at most 10 % of the rows / steps of each GPU test are ambiguous
    (printed; a condition on the chosen seeds, which only the reference decides);
  * each bound rejects an emulation with one mistake: a softmax without the max-subtraction, a top-k-off denominator over the
    candidate list only, a nucleus cut one candidate off.
"""
import os

import numpy as np
import pytest
import torch

import decode_tail_cases as dc
import fp64_bounds as fb
from oracle import decode_tail as dt
from oracle import models as om

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SAMPLER_VS = (1, 50, 255, 256, 257, 1024, 1025, 32001)


def _run_sampler_cases(cases, tag, **mutant):
    worst, amb, rows = 0.0, 0, 0
    for c in cases:
        for b in range(c["logits"].shape[0]):
            out = dc.emulate_sampler_row(c, b, **mutant)
            r, a = fb.check_sampler_row(c, b, out, f"{c['name']}[{b}]")
            worst, amb, rows = max(worst, r), amb + int(a), rows + 1
    print(f"emulation err/bound sampler {tag}: {worst:.3f}; ambiguous {amb}/{rows}")
    assert worst < 1.0
    assert amb <= 0.10 * rows, f"{tag}: {amb} of {rows} rows ambiguous"
    return worst


# ---- the references against what the project already trusts ---------------------------------------------------------------------
def test_sampler_reference_reproduces_hf_golden():
    a = np.load(os.path.join(GOLDEN, "sampling.npz"))
    for i in range(7):
        temp, k, p, pen = a[f"knobs_{i}"].tolist()
        for b in range(3):
            scores = dt.sampler_scores(a[f"logits_{i}"][b], a[f"prev_{i}"][b].tolist(), pen, temp)
            ref = dt.SamplerRef(scores, int(k), np.float32(p))
            want = a[f"probs_{i}"][b]
            kept = np.nonzero(want > 0)[0]
            n = len(kept)                                      # (one golden row puts a tail mass exactly on 1 - top_p)
            assert ref.keep_lo <= n <= ref.keep_hi and (n == ref.keep or not ref.cut_determinate), (i, b)
            if n == ref.n or scores[ref.cand[n - 1]] != scores[ref.cand[n]]:
                assert sorted(ref.cand[:n].tolist()) == kept.tolist(), (i, b)
            else:                                              # the cut falls among bit-equal scores: HF's sort picks any of them
                assert scores[kept].tolist() == scores[np.sort(ref.cand[:n])].tolist() or \
                    sorted(scores[kept].tolist()) == sorted(scores[ref.cand[:n]].tolist()), (i, b)
            _, _, p64, e_p = ref.kept(n)
            # HF's own float32 softmax carries the same kind of error as the kernel's: twice the bound separates the two
            hf = np.sort(want[kept])[::-1]
            assert np.all(np.abs(hf - np.sort(p64)[::-1]) <= 2 * np.sort(e_p)[::-1] + 1e-7 * hf), (i, b)


def test_sampler_reference_agrees_with_float32_restatement():
    g = torch.Generator().manual_seed(5)
    for V, temp, k, p, pen in ((32001, 0.8, 50, 0.9, 1.0), (32001, 0.8, 50, 0.9, 1.3), (777, 1.0, 5, 0.5, 1.0), (260, 1.5, 200, 0.99, 1.2),
                               (32001, 1.0, 1000, 1.0, 1.0), (32001, 0.6, 1, 1.0, 1.5)):
        logits = (torch.randn(5, V, generator=g) * 3.0).numpy()
        prev = torch.randint(0, V, (5, 6), generator=g).numpy()
        for b in range(5):
            oi, op = om.sample_filter(logits[b], prev[b].tolist(), pen, temp, k, p)
            ref = dt.SamplerRef(dt.sampler_scores(logits[b], prev[b].tolist(), pen, temp), k, np.float32(p))
            assert ref.keep_lo <= len(oi) <= ref.keep_hi
            assert oi.tolist() == ref.cand[:len(oi)].tolist()
            _, _, p64, e_p = ref.kept(len(oi))
            assert np.all(np.abs(op - p64) <= e_p), (V, b, float((np.abs(op - p64) / e_p).max()))


def test_beam_reference_agrees_with_float32_bookkeeping():
    """Whole searches: BeamBookkeeping (float32, its own history) and BeamStepRef (float64, one step at a time from the state
    the f32 emulation left) choose the same parents and tokens at every determinate step."""
    for name, Bn, K, V, T, eos, lp, pen, seed in dc.beam_search_setups():
        bk = om.BeamBookkeeping(Bn, K, T, eos, lp, pen)
        model = dc.SearchLogits(Bn, K, V, eos, seed)
        st = dc.beam_state(Bn, K, T, V - 1)
        det = 0
        for s in range(T):
            lg = model.logits()
            rows = lg.shape[0] // Bn
            full = lg if rows == K else np.repeat(lg, K, 0)
            parents, toks = bk.step(torch.from_numpy(full))
            for b in range(Bn):
                old = dc.beam_row_view(st, b)
                ref = dt.BeamStepRef(lg[b * rows:(b + 1) * rows], V, K, T, s, eos, lp, pen, old["run_score"], old["run_seq"], old["fin_score"],
                                     old["fin_seq"], old["fin_len"], old["fin_flag"], old["unsat"])
                out = dc.emulate_beam_row(lg[b * rows:(b + 1) * rows], V, K, T, s, eos, lp, pen, old)
                if ref.determinate and s + 1 < T:
                    det += 1
                    assert (parents.view(Bn, K)[b] - b * K).tolist() == ref.parent.tolist(), (name, s, b)
                    assert toks.view(Bn, K)[b].tolist() == ref.next_ids.tolist(), (name, s, b)
                    assert int(bk.open[b]) == ref.unsat, (name, s, b)
                for k2, v in out.items():
                    if k2 in st:
                        st[k2][b] = v
            model.advance(parents.numpy(), toks.numpy())
        assert det >= (T - 1) * Bn * 0.8, (name, det)


# ---- the emulation inside the bounds on every GPU-test input, the ambiguous share ---------------------------------------------
@pytest.mark.parametrize("V", SAMPLER_VS)
def test_sampler_emulation_within_bounds_on_grid(V):
    _run_sampler_cases(dc.sampler_test_cases(V), f"grid V={V}")


def test_sampler_emulation_within_bounds_on_planted_cases():
    _run_sampler_cases([dc.sampler_large_case()], "V=156032")
    _run_sampler_cases([dc.sampler_bookkeeping_case()], "bookkeeping")
    _run_sampler_cases([dc.sampler_greedy_penalty_case()], "greedy+penalty")
    _run_sampler_cases(dc.sampler_overflow_cases(), "overflow")
    _run_sampler_cases([dc.sampler_hot_case()], "hot scores")


def test_a_u_on_a_cdf_step_admits_both_neighbours():
    c = dc.sampler_test_cases(257)[-1]
    scores = dt.sampler_scores(c["logits"][0, :c["V"]], c["tokens"][0, :c["step"]], c["pen"], c["temp"])
    ref = dt.SamplerRef(scores, c["top_k"], c["top_p"])
    assert len(ref.justified_picks(c["u"][0])) == 2 and not ref.pick(c["u"][0])[1]


def _run_beam_cases(cases, tag, **mutant):
    worst, amb, rows = 0.0, 0, 0
    for c in cases:
        rpb = c["rows"]
        for b in range(c["B"]):
            old = dc.beam_row_view(c["state"], b)
            lg = c["logits"][b * rpb:(b + 1) * rpb]
            ref = dc.beam_row_ref(c, lg, old)
            out = dc.emulate_beam_row(lg, c["V"], c["K"], c["T"], c["step"], c["eos"], c["lp"], c["pen"], old, **mutant)
            r, a = fb.check_beam_row(ref, out, old, f"{c['name']}[{b}]")
            worst, amb, rows = max(worst, r), amb + int(a), rows + 1
    print(f"emulation err/bound beam {tag}: {worst:.3f}; ambiguous {amb}/{rows}")
    assert worst < 1.0
    assert amb <= 0.10 * rows, f"{tag}: {amb} of {rows} steps ambiguous"


def test_beam_emulation_within_bounds_on_single_launches():
    cases = dc.beam_single_cases()
    _run_beam_cases(cases, "single launches")
    # what the crafted states are for, as the reference sees it
    seen = set()
    for c in cases:
        for b in range(c["B"]):
            old = dc.beam_row_view(c["state"], b)
            ref = dc.beam_row_ref(c, c["logits"][b * c["rows"]:(b + 1) * c["rows"]], old)
            ranks = [j for j in range(ref.NC) if int(ref.ci[j]) % c["V"] in ref.eos]
            seen |= {"eos<K"} if any(j < c["K"] for j in ranks) else set()
            seen |= {"eos>=K"} if any(j >= c["K"] for j in ranks) else set()
            seen |= {"closed"} if not ref.row_open else set()
            full = bool(np.all(old["fin_flag"] == 1))
            cand_in = any(s >= c["K"] for s in ref.fin_src)
            seen |= {"displaced"} if full and cand_in else set()
            seen |= {"not displaced"} if full and ref.row_open and not cand_in and any(ref.stops[:c["K"]]) else set()
            seen |= {"partly filled"} if 0 < int(old["fin_flag"].sum()) < c["K"] else set()
            seen |= {"-inf kept"} if np.isneginf(ref.cv).any() else set()
    assert seen == {"eos<K", "eos>=K", "closed", "displaced", "not displaced", "partly filled", "-inf kept"}, seen


def _emulated_search(name, Bn, K, V, T, eos, lp, pen, seed, **mutant):
    model = dc.SearchLogits(Bn, K, V, eos, seed)
    st = dc.beam_state(Bn, K, T, V - 1)
    worst, amb, steps = 0.0, 0, 0
    for s in range(T):
        lg = model.logits()
        rows = lg.shape[0] // Bn
        par, tok = [], []
        for b in range(Bn):
            old = dc.beam_row_view(st, b)
            old = {k: (np.array(v) if k != "unsat" else v) for k, v in old.items()}
            p = dict(V=V, K=K, T=T, step=s, eos=eos, lp=lp, pen=pen)
            ref = dc.beam_row_ref(p, lg[b * rows:(b + 1) * rows], old)
            out = dc.emulate_beam_row(lg[b * rows:(b + 1) * rows], V, K, T, s, eos, lp, pen, old, **mutant)
            r, a = fb.check_beam_row(ref, out, old, f"{name} step {s} row {b}")
            worst, amb, steps = max(worst, r), amb + int(a), steps + 1
            for k2, v in out.items():
                if k2 in st:
                    st[k2][b] = v
            par += (out["parent"] + b * K).tolist()
            tok += out["next_ids"].tolist()
        model.advance(np.array(par), np.array(tok))
    print(f"emulation err/bound beam {name}: {worst:.3f}; ambiguous {amb}/{steps}")
    assert worst < 1.0 and amb <= 0.10 * steps


@pytest.mark.parametrize("setup", dc.beam_search_setups(), ids=lambda s: s[0])
def test_beam_emulation_within_bounds_on_whole_searches(setup):
    _emulated_search(*setup)


# ---- the bounds reject a kernel with one mistake ------------------------------------------------------------------------------------
def test_bounds_reject_a_softmax_without_max_subtraction():
    with pytest.raises(AssertionError):
        _run_sampler_cases([dc.sampler_hot_case()], "mutant: no max", no_max=True)
    hot = [c for c in dc.beam_single_cases() if c["name"] == "hot-logits"]
    with pytest.raises(AssertionError):
        _run_beam_cases(hot, "mutant: no max", no_max=True)


def test_bounds_reject_a_denominator_over_the_candidates_only():
    # (the kept probabilities are renormalised, so the row's denominator shows only where the nucleus cut reads it: top_p < 1)
    cases = [c for c in dc.sampler_grid_cases(32001) if c["top_k"] == 32001 and c["top_p"] == 0.9]
    assert cases
    for c in cases:
        with pytest.raises(AssertionError):
            _run_sampler_cases([c], "mutant: denominator", wrong_denominator=True)


def test_bounds_reject_a_nucleus_cut_one_off():
    cases = [c for V in (50, 1025, 32001) for c in dc.sampler_grid_cases(V) if c["top_p"] == 0.9 and c["top_k"] >= 50]
    assert cases
    for c in cases:
        with pytest.raises(AssertionError):
            _run_sampler_cases([c], "mutant: cut", cut_off_by_one=True)

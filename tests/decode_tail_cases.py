"""Inputs shared by test_decode_tail_bounds.py (CPU) and test_gpu_decode_tail_exact.py (GPU), and the numpy float32 emulations
of sample_eos_kernel / beam_step_kernel in the kernels' summation order that the CPU module runs over those inputs.  Not a
test module: plain functions over numpy arrays, deterministic (every case seeds its own generator).

A sampler case is a dict: logits f32 [B, ldl] (columns V.. hold +inf / NaN), V, ldw, tokens int32 [B, width] (the out_tokens
buffer before the launch: columns < step are the previous tokens), step, temp, top_k, top_p, pen, u f32 [B], eos (e1, e2), pad,
finished int32 [B], sentinel (the f32 written where the launch must not write).
A beam case is a dict: logits f32 [B * rows, ldl], V, K, T, step, eos, lp, pen, rows and the incoming state arrays."""
import numpy as np

from oracle import decode_tail as dt

SENTINEL = np.float32(-12345.5)
ONE_BELOW = np.nextafter(np.float32(1.0), np.float32(0.0))


# ---- sampler cases ------------------------------------------------------------------------------------------------------------
def _pitch(rows, V, pad_cols, rng):
    """[B, V] -> [B, V + pad_cols] with +inf and NaN in the pad columns."""
    Bn = rows.shape[0]
    out = np.empty((Bn, V + pad_cols), np.float32)
    out[:, :V] = rows
    if pad_cols:
        out[:, V:] = np.where(rng.random((Bn, pad_cols)) < 0.5, np.inf, np.nan).astype(np.float32)
    return out


def _case(name, rows, *, step, width, temp, top_k, top_p, pen, u, tokens=None, eos=(-1, -1), pad=0, finished=None, pad_cols=0,
          ldw_extra=0, seed=0):
    rng = np.random.default_rng(seed)
    Bn, V = rows.shape
    tk = np.full((Bn, width), 7 % V, np.int32) if tokens is None else tokens.astype(np.int32)
    return dict(name=name, logits=_pitch(rows.astype(np.float32), V, pad_cols, rng), V=V, ldw=V + ldw_extra, tokens=tk, step=step,
                temp=temp, top_k=top_k, top_p=top_p, pen=pen, u=np.asarray(u, np.float32), eos=eos, pad=pad,
                finished=np.zeros(Bn, np.int32) if finished is None else np.asarray(finished, np.int32), sentinel=SENTINEL)


def _planted_rows(V, top_k, rng):
    """Five rows of different character: Gaussian; peaked (a nucleus of one); nearly flat (a wide nucleus: every candidate at
    top_p = 1); ties straddling the top-k cut; NaN and -inf among Gaussian logits."""
    r = (rng.standard_normal((5, V)) * 3.0).astype(np.float32)
    r[1, rng.integers(0, V)] = 40.0
    r[2] = (rng.standard_normal(V) * 0.01).astype(np.float32)
    k = min(top_k, V)
    srt = np.sort(r[3])[::-1]
    if V >= 4:
        cut = srt[min(k, V) - 1]
        where = rng.choice(V, size=min(4, V), replace=False)
        r[3, where] = cut                                      # several tokens bit-equal to the k-th value
    if V >= 8:
        where = rng.choice(V, size=4, replace=False)
        r[4, where[:2]] = np.nan
        r[4, where[2:]] = -np.inf
    return r


def _history(V, Bn, width, step, pad, rng, rows):
    """Previous tokens with duplicates, -1, ids >= V, the pad id, and hits on a negative, a positive and an exactly-zero logit."""
    tk = rng.integers(0, V, size=(Bn, width)).astype(np.int32)
    if step >= 8:
        tk[:, 1] = tk[:, 0]
        tk[:, 2] = -1
        tk[:, 3] = V
        tk[:, 4] = V + 5
        tk[:, 5] = pad
        for b in range(Bn):
            fin = np.nonzero(np.isfinite(rows[b]))[0]
            neg, pos = fin[rows[b, fin] < 0], fin[rows[b, fin] > 0]
            if neg.size:
                tk[b, 6] = neg[0]
            if pos.size:
                tk[b, 7] = pos[-1]
            if V > 3 and step >= 9:
                z = int(rng.integers(0, V))
                if np.isfinite(rows[b, z]) and rows[b, z] != rows[b].max():
                    rows[b, z] = 0.0
                    tk[b, 8] = z
    tk[:, step:] = 7 % V                                       # what the buffer holds past the previous tokens (must stay)
    return tk


def sampler_grid_cases(V):
    """Every (top_k, top_p) of the grid {1, 2, 50, 1024, V} x {1, 0.9, 1e-6} at vocabulary V, each as a B = 1 launch at step 0 (no previous tokens, dense
    rows) and as a B = 5 launch at step 300 (n_prev > 256, wider pitches, penalty 1.3, the five planted rows)."""
    cases = []
    ks = sorted({k for k in (1, 2, 50, 1024, V) if k <= V})
    for ik, k in enumerate(ks):
        for ip, p in enumerate((1.0, 0.9, 1e-6)):
            seed = V * 100 + ik * 10 + ip
            rng = np.random.default_rng(seed)
            row = (rng.standard_normal((1, V)) * 3.0).astype(np.float32)
            cases.append(_case(f"V{V}-k{k}-p{p}-B1", row, step=0, width=4, temp=0.8, top_k=k, top_p=p, pen=1.3,
                               u=rng.random(1), seed=seed))
            rows = _planted_rows(V, k, rng)
            tk = _history(V, 5, 320, 300, 0, rng, rows)
            u = np.array([0.0, ONE_BELOW, rng.random(), rng.random(), rng.random()], np.float32)
            cases.append(_case(f"V{V}-k{k}-p{p}-B5", rows, step=300, width=320, temp=0.7, top_k=k, top_p=p, pen=1.3, u=u,
                               tokens=tk, pad_cols=5, ldw_extra=3, seed=seed + 1))
    return cases


def with_u_on_a_cdf_step(case, b=0):
    """A copy of `case` whose row b draws the f32 nearest to an inner CDF step of its float64 distribution: within the bound of
    that step, so either neighbour is a justified pick (the row is ambiguous by construction)."""
    c = dict(case)
    scores = dt.sampler_scores(case["logits"][b, :case["V"]], case["tokens"][b, :case["step"]], case["pen"], case["temp"])
    ref = dt.SamplerRef(scores, case["top_k"], case["top_p"])
    cdf, _, _, _ = ref.kept()
    assert len(cdf) >= 3
    u = case["u"].copy()
    u[b] = np.float32(cdf[len(cdf) // 2 - 1])
    c["u"], c["name"] = u, case["name"] + "-u@cdf"
    return c


def sampler_test_cases(V):
    """The grid at V plus (V >= 50) one launch whose first row draws on a CDF step."""
    cases = sampler_grid_cases(V)
    if V >= 50:
        wide = [c for c in cases if c["top_p"] == 1.0 and c["name"].endswith("B5")][-1]
        cases.append(with_u_on_a_cdf_step(wide, b=0))
    return cases


def sampler_large_case():
    V = 156032
    rng = np.random.default_rng(156032)
    rows = _planted_rows(V, 50, rng)
    tk = _history(V, 5, 320, 300, 0, rng, rows)
    u = np.array([0.0, ONE_BELOW, rng.random(), rng.random(), rng.random()], np.float32)
    return _case("V156032-k50-p0.9-B5", rows, step=300, width=320, temp=0.7, top_k=50, top_p=0.9, pen=1.1, u=u, tokens=tk,
                 pad_cols=8, ldw_extra=8, seed=1)


def sampler_bookkeeping_case():
    """top_k = 1 on rows with one clear maximum: row 0 was finished (emits pad whatever it draws), row 1 draws eos_id, row 2
    draws eos_id2, row 3 draws the pad id (not an EOS: stays unfinished), row 4 an ordinary token; row 5 finished AND drawing EOS."""
    V, pad, e1, e2 = 257, 9, 100, 256
    rng = np.random.default_rng(5)
    rows = (rng.standard_normal((6, V))).astype(np.float32)
    for b, t in enumerate((3, e1, e2, pad, 200, e1)):
        rows[b, t] = 9.0
    return _case("bookkeeping", rows, step=2, width=5, temp=1.0, top_k=1, top_p=1.0, pen=1.0, u=rng.random(6), eos=(e1, e2), pad=pad,
                 finished=[1, 0, 0, 0, 0, 1], pad_cols=3, ldw_extra=1, seed=5)


def sampler_greedy_penalty_case():
    """HF greedy search under a repetition penalty = temperature 1, top_k 1, top_p 1, u 0: the lowest-id arg-max of the
    PENALISED row.  Row 0: the raw maximum was generated before and falls behind; row 1: two tokens tie for the penalised
    maximum bit for bit (the lower id wins; the candidate list holds both); row 2: a negative maximum that the penalty lowers."""
    V = 32001
    rng = np.random.default_rng(77)
    rows = (rng.standard_normal((3, V)) * 2.0).astype(np.float32)
    rows = np.minimum(rows, np.float32(6.0))
    tk = rng.integers(0, V, size=(3, 16)).astype(np.int32)
    rows[0, 31000], rows[0, 12] = 9.0, 8.0
    tk[0, 0] = 31000                                           # 9 / 1.5 = 6 < 8
    rows[1, 20000], rows[1, 500], rows[1, 31999] = 12.0, 8.0, 8.0
    tk[1, 3] = 20000                                           # 12 / 1.5 = 8: a three-way tie at 8 -> token 500
    rows[2] = -np.abs(rows[2]) - np.float32(1.0)
    rows[2, 40], rows[2, 41] = -0.5, -0.7
    tk[2, 2] = 40                                              # -0.5 * 1.5 = -0.75 < -0.7
    tk[:, 6:] = 7
    return _case("greedy+penalty", rows, step=6, width=16, temp=1.0, top_k=1, top_p=1.0, pen=1.5, u=np.zeros(3), tokens=tk, seed=77)


def sampler_overflow_cases():
    """More than SAMPLE_CAP tokens at or above the cut (include/icl_hip.h: every token above it, then the tied ones by ascending
    id).  One row per launch variant, V = 32001; rows of the same launch differ in u."""
    V = 32001
    cases = []
    us = np.array([0.0, 0.37, ONE_BELOW], np.float32)

    def three(row):
        return np.repeat(row[None], 3, 0)
    rng = np.random.default_rng(2000)
    row = (rng.standard_normal(V) * 0.5 - 6.0).astype(np.float32)         # everything else far below
    row[rng.choice(V - 10, size=2000, replace=False)] = 1.0
    row[V - 10:] = np.linspace(2.0, 3.0, 10, dtype=np.float32)            # the ten strictly above, at the highest ids
    cases.append(_case("ten-above-2000-ties-k50", three(row), step=0, width=4, temp=1.0, top_k=50, top_p=1.0, pen=1.0, u=us))
    cases.append(_case("ten-above-2000-ties-k50-p0.9", three(row), step=0, width=4, temp=1.0, top_k=50, top_p=0.9, pen=1.0, u=us))
    flat = np.full(V, 0.25, np.float32)
    cases.append(_case("all-equal-k1", three(flat), step=0, width=4, temp=1.0, top_k=1, top_p=1.0, pen=1.0, u=us))
    cases.append(_case("all-equal-k50", three(flat), step=0, width=4, temp=0.5, top_k=50, top_p=0.9, pen=1.0, u=us))
    masked = np.full(V, -np.inf, np.float32)
    masked[[31990, 17, 20000]] = [1.0, 0.5, 2.0]
    cases.append(_case("masked-3-finite-k50", three(masked), step=0, width=4, temp=1.0, top_k=50, top_p=1.0, pen=1.0, u=us))
    row = (rng.standard_normal(V) * 0.5 - 8.0).astype(np.float32)
    row[rng.choice(V - 1000, size=3000, replace=False)] = 0.0             # 3000 ties at the 1024th value
    row[V - 1000:] = (1.0 + rng.random(1000) * 2.0).astype(np.float32)    # 1000 strictly above, at the highest ids
    cases.append(_case("topk-off-3000-ties", three(row), step=0, width=4, temp=1.0, top_k=V, top_p=1.0, pen=1.0, u=us))
    cases.append(_case("topk-off-3000-ties-p0.9", three(row), step=0, width=4, temp=1.0, top_k=V, top_p=0.9, pen=1.0, u=us))
    # greedy with penalty on a row whose maximum sits above a flat row: must be the arg-max, never a tied token
    row = np.full(V, 1.0, np.float32)
    row[V - 3] = 5.0
    cases.append(_case("greedy-over-flat", three(row), step=0, width=4, temp=1.0, top_k=1, top_p=1.0, pen=1.0, u=np.zeros(3)))
    return cases


def sampler_hot_case():
    """Scores far above expf's overflow (x / temperature ~ 300): only the max-subtraction keeps the softmax finite."""
    rng = np.random.default_rng(31)
    rows = (rng.standard_normal((5, 1025)) * 6.0).astype(np.float32)
    return _case("hot-scores", rows, step=0, width=4, temp=0.05, top_k=50, top_p=0.9, pen=1.0, u=rng.random(5), seed=31)


# ---- sampler emulation (f32, the kernel's order) ----------------------------------------------------------------------------------
def _block_sum_f32(vals):
    """256 threads: thread t adds elements t, t + 256, .. in series; a 6-level xor butterfly per wave of 64; (w0 + w1) + (w2 + w3)."""
    n = len(vals)
    pad = (-n) % 256
    v = np.concatenate([np.asarray(vals, np.float32), np.zeros(pad, np.float32)]).reshape(-1, 256)
    part = np.zeros(256, np.float32)
    for r in range(v.shape[0]):
        part = (part + v[r]).astype(np.float32)
    lanes = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        part = (part + part[lanes ^ o]).astype(np.float32)
    return np.float32(np.float32(part[0] + part[64]) + np.float32(part[128] + part[192]))


def emulate_sampler_row(case, b, cap=1024, dbg_cap=1024, no_max=False, wrong_denominator=False, cut_off_by_one=False):
    """The outputs of one sampler row in float32, operation by operation as sample_eos_kernel orders them.  The three switches
    plant the mistakes the bounds must reject: a softmax without the max-subtraction, a top-k-off denominator over the candidate
    list only, a nucleus cut one candidate off."""
    f32 = np.float32
    V, step = case["V"], case["step"]
    w = dt.sampler_scores(case["logits"][b, :V], case["tokens"][b, :step], case["pen"], case["temp"])
    cand = dt.sampler_candidates(w, case["top_k"], cap)
    n = len(cand)
    full = case["top_k"] >= V
    top = f32(0.0) if no_max else w[cand[0]]
    with np.errstate(all="ignore"):
        x = w[cand]
        e = np.where(np.isnan(x), f32(0.0), np.exp((x - top).astype(f32))).astype(f32)
        if full and not wrong_denominator:
            ex = np.where(np.isnan(w), f32(0.0), np.exp((w - top).astype(f32))).astype(f32)
            denom = _block_sum_f32(ex)
        else:
            denom = _block_sum_f32(e)
        p = (e / denom).astype(f32)
    top_p = f32(case["top_p"])
    thr = f32(f32(1.0) - top_p)
    keep = n
    if top_p < 1.0 and full:
        before, keep = p[0], 1
        for j in range(1, n):
            if not f32(f32(1.0) - before) > thr:
                break
            before = f32(before + p[j])
            keep = j + 1
    elif top_p < 1.0:
        tail, keep = f32(0.0), 1
        for j in range(n - 1, 0, -1):
            tail = f32(tail + p[j])
            if tail > thr:
                keep = j + 1
                break
    if cut_off_by_one:
        keep = keep + 1 if keep < n else max(1, keep - 1)
    total = f32(0.0)
    for j in range(keep):
        total = f32(total + p[j])
    target = f32(f32(case["u"][b]) * total)
    acc, pick = f32(0.0), keep - 1
    for j in range(keep):
        acc = f32(acc + p[j])
        if acc > target:
            pick = j
            break
    fin = int(case["finished"][b])
    tok = case["pad"] if fin else int(cand[pick])
    if tok in [t for t in case["eos"] if t >= 0]:
        fin = 1
    work = np.full(case["ldw"], case["sentinel"], f32)
    work[:V] = w
    ids = np.full(dbg_cap, -1, np.int32)
    probs = np.full(dbg_cap, case["sentinel"], f32)
    ids[:keep] = cand[:keep]
    with np.errstate(all="ignore"):
        probs[:keep] = (p[:keep] / total).astype(f32)
    toks = case["tokens"][b].copy()
    toks[step] = tok
    return dict(work=work, ids=ids, probs=probs, count=keep, next_id=tok, tokens=toks, finished=fin)


# ---- beam cases -----------------------------------------------------------------------------------------------------------------
def beam_state(Bn, K, T, pad):
    """The initial state of include/icl_hip.h."""
    st = dict(run_score=np.full((Bn, K), -1.0e9, np.float32), run_seq=np.full((Bn, K, T), pad, np.int32),
              fin_score=np.full((Bn, K), -1.0e9, np.float32), fin_seq=np.full((Bn, K, T), pad, np.int32),
              fin_len=np.zeros((Bn, K), np.int32), fin_flag=np.zeros((Bn, K), np.int32), unsat=np.ones(Bn, np.int32))
    st["run_score"][:, 0] = 0.0
    return st


def _crafted_state(Bn, K, T, V, step, pad, lp, rng, filled, closed=()):
    """A state no previous launch need have left: running beams with plausible scores and histories (duplicates and the pad id
    among the tokens), `filled[b]` finished slots per row with scores around the running ones, rows in `closed` with unsat = 0."""
    st = beam_state(Bn, K, T, pad)
    if step == 0:
        return st
    for b in range(Bn):
        st["run_score"][b] = -np.sort(rng.random(K).astype(np.float32) * 2.0 * step * 0.4 + 0.1 * step)
        seq = rng.integers(0, V, size=(K, T)).astype(np.int32)
        seq[:, step:] = pad
        if step >= 3:
            seq[:, 1] = seq[:, 0]
            seq[:, 2] = pad
        st["run_seq"][b] = seq
        nf = filled[b % len(filled)]
        for i in range(min(nf, K)):
            L = int(rng.integers(1, step + 1))
            st["fin_seq"][b, i, :L] = rng.integers(0, V, size=L)
            st["fin_len"][b, i], st["fin_flag"][b, i] = L, 1
        sc = -(rng.random(min(nf, K)).astype(np.float32) * 1.5 + 0.2) * step * 0.5 / np.float32(float(step) ** lp)
        st["fin_score"][b, :min(nf, K)] = -np.sort(-sc)
        if b in closed:
            st["unsat"][b] = 0
    return st


def _beam_case(name, K, V, T, step, eos, lp, pen, rows, Bn, seed, filled=(0,), closed=(), pad_cols=0, scale=2.0, pad=None, tweak=None):
    rng = np.random.default_rng(seed)
    pad = V - 1 if pad is None else pad
    lg = (rng.standard_normal((Bn * rows, V)) * scale).astype(np.float32)
    st = _crafted_state(Bn, K, T, V, step, pad, lp, rng, filled, closed)
    c = dict(name=name, K=K, V=V, T=T, step=step, eos=eos, lp=lp, pen=pen, rows=rows, B=Bn, state=st)
    if tweak:
        tweak(lg, st, rng)
    c["logits"] = _pitch(lg, V, pad_cols, rng)
    if pad_cols:
        c["logits"][:, V:] = np.inf
    return c


def beam_single_cases():
    cases = []
    # V == NC: every continuation of beam 0 is kept at step 0; later steps draw from all beams
    cases.append(_beam_case("K1-V2", 1, 2, 4, 0, 0, 1.0, 1.0, 1, 2, 1))
    cases.append(_beam_case("K1-V2-step2", 1, 2, 4, 2, 0, 1.0, 1.6, 1, 2, 2, filled=(0, 1)))
    cases.append(_beam_case("K4-V8", 4, 8, 5, 0, 3, 1.0, 1.0, 1, 3, 3))
    cases.append(_beam_case("K4-V8-step3", 4, 8, 5, 3, 3, 2.0, 1.6, 4, 3, 4, filled=(0, 2, 4), closed=(2,)))
    cases.append(_beam_case("K2-V6-2eos", 2, 6, 4, 0, (0, 5), 1.0, 1.0, 1, 2, 5))
    cases.append(_beam_case("K2-V6-2eos-step2", 2, 6, 4, 2, (0, 5), -1.0, 1.6, 2, 3, 6, filled=(1, 2, 0)))
    for V in (40, 255, 257, 32001):
        for i, (lp, pen) in enumerate(((0.0, 1.0), (1.0, 1.6), (2.0, 1.6), (-1.0, 1.0))):
            K = (3, 4, 8, 2)[i]
            step = (0, 4, 2, 5)[i]
            cases.append(_beam_case(f"V{V}-K{K}-lp{lp}-pen{pen}-s{step}", K, V, 8, step, (5, 17) if i == 2 else 5, lp, pen, K if step else 1,
                                    3, V * 10 + i, filled=(0, K // 2, K), closed=(1,) if i == 1 else (), pad_cols=7 if i % 2 else 0))
    # K = 8, T = 64 at the first and the last steps (step 63: the length limit stops everything)
    for step in (0, 1, 62, 63):
        cases.append(_beam_case(f"K8-T64-s{step}", 8, 300, 64, step, 7, 1.0, 1.6, 8, 2, 640 + step, filled=(3, 8), pad_cols=4))

    def few_finite(lg, st, rng):                             # fewer than NC finite continuations in the row: -inf ties go low
        lg[:] = -np.inf
        lg[:, 3] = 0.5
        lg[1:, 30] = 0.1
        lg[1, 11] = np.nan
    cases.append(_beam_case("few-finite-s0", 4, 40, 6, 0, 9, 1.0, 1.0, 1, 2, 71, tweak=few_finite))
    cases.append(_beam_case("few-finite-s2", 2, 40, 6, 2, 9, 1.0, 1.6, 2, 2, 72, filled=(1,), tweak=few_finite))

    def eos_first(lg, st, rng):                              # EOS is every beam's best continuation: rank < K
        lg[:, 5] = lg.max() + 3.0
    def displaced(lg, st, rng):                              # every slot holds a poor hypothesis: the new ones take them over
        eos_first(lg, st, rng)
        st["fin_score"][:] = np.float32([-30, -40, -50, -60])

    def kept(lg, st, rng):                                   # every slot holds a better one than any candidate: nothing moves
        eos_first(lg, st, rng)
        st["fin_score"][:] = np.float32([-0.001, -0.002, -0.003, -0.004])
    cases.append(_beam_case("eos-rank0-displaces", 4, 257, 8, 3, 5, 1.0, 1.0, 4, 2, 81, filled=(4,), tweak=displaced))
    cases.append(_beam_case("eos-rank0-does-not-displace", 4, 257, 8, 3, 5, 1.0, 1.0, 4, 2, 82, filled=(4,), tweak=kept))

    def eos_late(lg, st, rng):                               # step 0: EOS between the (K+1)-th and (K+2)-th best -> rank >= K
        for r in range(lg.shape[0]):
            s = np.sort(lg[r])[::-1]
            lg[r, 5] = (s[5] + s[6]) / 2
    cases.append(_beam_case("eos-rank-ge-K", 4, 257, 8, 0, 5, 1.0, 1.0, 1, 2, 83, tweak=eos_late))

    def hot(lg, st, rng):                                    # logits past expf's overflow: only x - max keeps the log-sum finite
        lg *= 60.0
    cases.append(_beam_case("hot-logits", 4, 257, 8, 3, 5, 1.0, 1.0, 4, 2, 84, filled=(2,), tweak=hot))
    return cases


def beam_search_setups():
    """(name, Bn, K, V, T, eos, lp, pen, seed) of the two whole searches run on the kernel's (or the emulation's) own history."""
    return [("search-K4-V257", 3, 4, 257, 6, 17, 1.0, 1.6, 11), ("search-K8-V32001-2eos", 2, 8, 32001, 5, (2, 31999), 2.0, 1.0, 12)]


class SearchLogits:
    """A tiny recurrent stand-in for the decoder: logits depend on each beam's history along the chosen parents; peaked EOS
    columns and one bit-equal pair of tokens per beam make EOS and exact ties part of the race."""

    def __init__(self, Bn, K, V, eos, seed):
        rng = np.random.default_rng(seed)
        Hd = 12
        self.A = rng.standard_normal((Hd, Hd)) * 0.6
        self.E = rng.standard_normal((V, Hd))
        self.Uo = rng.standard_normal((Hd, V)) * 1.5
        for e in (eos if isinstance(eos, tuple) else (eos,)):
            self.Uo[:, e] += 0.8
        self.hid = rng.standard_normal((Bn, Hd))
        self.Bn, self.K, self.V = Bn, K, V

    def logits(self):
        lg = (self.hid @ self.Uo).astype(np.float32)
        if self.V > 20:
            lg[:, 7] = lg[:, 11]
        return lg

    def advance(self, parent_abs, tokens):
        rows = self.hid if self.hid.shape[0] == self.Bn * self.K else np.repeat(self.hid, self.K, 0)
        self.hid = np.tanh(rows[parent_abs] @ self.A + self.E[tokens])


# ---- beam emulation (f32, the kernel's order) ---------------------------------------------------------------------------------------
def emulate_beam_row(logits, V, K, T, step, eos, lp, pen, old, no_max=False):
    """One batch row of beam_step_kernel in float32.  `logits` [rows, >= V]; `old`: the row's incoming state.  Returns the
    row's outgoing state, next_ids and parent (beam index inside the row)."""
    f32 = np.float32
    eos = [int(e) for e in (eos if isinstance(eos, (tuple, list)) else [eos]) if int(e) >= 0]
    NC = (3 if len(eos) > 1 else 2) * K
    x = np.asarray(logits, f32)[:, :V]
    if x.shape[0] == 1:
        x = np.repeat(x, K, 0)
    x = np.where(np.isnan(x), f32(-np.inf), x)
    lenpen = f32(float(step + 1) ** float(lp))
    pen = f32(pen)
    a = np.empty((K, V), f32)
    with np.errstate(all="ignore"):
        for k in range(K):
            m = x[k].max()
            if not m > -np.inf:
                m = f32(0.0)
            if no_max:
                m = f32(0.0)
            ls = f32(np.log(_block_sum_f32(np.exp((x[k] - m).astype(f32)).astype(f32))))
            lpk = np.where(x[k] > -np.inf, ((x[k] - m).astype(f32) - ls).astype(f32), f32(-np.inf)).astype(f32)
            if pen != f32(1.0) and step > 0:
                seen = np.unique([t for t in np.asarray(old["run_seq"])[k, :step].tolist() if 0 <= t < V]).astype(np.int64)
                if seen.size:
                    lpk[seen] = np.where(lpk[seen] < 0, lpk[seen] * pen, lpk[seen] / pen).astype(f32)
            a[k] = (lpk + f32(old["run_score"][k])).astype(f32)
    flat = a.reshape(-1)
    key = np.where(np.isnan(flat), -np.inf, flat).astype(np.float64)
    ci = np.lexsort((np.arange(K * V), -key))[:NC]
    cv = flat[ci]
    last = step + 1 >= T
    stops = np.array([last or (int(i) % V) in eos for i in ci])
    NEG = f32(-1.0e9)
    with np.errstate(all="ignore"):
        runv = np.where(stops, (cv + NEG).astype(f32), cv).astype(f32)
    used, run_src = [False] * NC, []
    for _ in range(K):
        best = -1
        for j in range(NC):
            if not used[j] and (best < 0 or runv[j] > runv[best]):
                best = j
        used[best] = True
        run_src.append(best)
    row_open = bool(old["unsat"])
    ms = [f32(v) for v in old["fin_score"]]
    mflag = [int(v) for v in old["fin_flag"]]
    with np.errstate(all="ignore"):
        for j in range(NC):
            just = bool(stops[j]) and j < K
            s = f32(cv[j] / lenpen)
            s = f32(s + (f32(-0.0) if row_open else NEG))
            s = f32(s + (f32(-0.0) if just else NEG))
            ms.append(s)
            mflag.append(1 if just else 0)
    mused, fin_src = [False] * (K + NC), []
    for _ in range(K):
        best = -1
        for j in range(K + NC):
            if not mused[j] and (best < 0 or ms[j] > ms[best]):
                best = j
        mused[best] = True
        fin_src.append(best)
    worst = min(ms[j] for j in fin_src)
    with np.errstate(all="ignore"):
        best_run = f32(runv[run_src[0]] / lenpen)
    any_ = any(bool(best_run > (worst if mflag[j] else NEG)) for j in fin_src)
    old_run, old_fin = np.asarray(old["run_seq"]), np.asarray(old["fin_seq"])
    out = dict(run_score=np.array([runv[j] for j in run_src], f32), next_ids=np.array([int(ci[j]) % V for j in run_src]),
               parent=np.array([int(ci[j]) // V for j in run_src]), fin_score=np.array([ms[j] for j in fin_src], f32),
               fin_flag=np.array([mflag[j] for j in fin_src]), unsat=int(row_open and any_),
               fin_len=np.array([int(old["fin_len"][j]) if j < K else step + 1 for j in fin_src]))
    out["run_seq"] = old_run[out["parent"]].copy()
    out["run_seq"][:, step] = out["next_ids"]
    fs = np.empty((K, T), np.int64)
    for i, j in enumerate(fin_src):
        if j < K:
            fs[i] = old_fin[j]
        else:
            c = int(ci[j - K])
            fs[i] = old_run[c // V]
            fs[i, step] = c % V
    out["fin_seq"] = fs
    return out


def beam_row_view(state, b):
    return {k: (v[b] if k != "unsat" else int(v[b])) for k, v in state.items()}


def beam_row_ref(case_or_params, logits_rows, old):
    c = case_or_params
    return dt.BeamStepRef(logits_rows, c["V"], c["K"], c["T"], c["step"], c["eos"], c["lp"], c["pen"], old["run_score"], old["run_seq"],
                          old["fin_score"], old["fin_seq"], old["fin_len"], old["fin_flag"], old["unsat"])

"""Float64 references of the two kernels that decide which token is emitted, one launch at a time:
`sample_eos_kernel` (csrc/sampling.hip) and `beam_step_kernel` (csrc/beam.hip).  Unlike `oracle.models.sample_filter` and
`BeamBookkeeping` (float32 restatements that sum in the kernels' own order, kept for the HF golden tests) nothing here
follows the kernels' arithmetic: sums are float64 over the whole set, and each reference comes with the error bound of the
kernel's f32 value, derived below, so that a test can say which outputs are determined and which hang on a rounding.

u = 2^-24 is the unit roundoff of f32.  EXPF_REL / LOGF_REL: the HIP math API documentation lists expf and logf at 1 ulp
maximum error; both are DOUBLED here (2 ulp = 2^-22 relative), which also covers the second-order terms the first-order
derivations below drop.

Sampler (per row)
  scores       two f32 operations, (x < 0 ? x * pen : x / pen) / temperature for tokens seen before, x / temperature otherwise:
               IEEE operations, reproduced bit for bit by numpy float32 (`sampler_scores`).
  candidates   from those f32 values the set and its order are exact: score descending, NaN below -inf, then token id
               ascending; every token tied with the top_k-th stays; more than SAMPLE_CAP of them: the first SAMPLE_CAP of that
               order, i.e. every token above the cut, then the tied ones by ascending id (`sampler_candidates`).
  mass         d_j = s_j - s_0, e_j = exp(d_j) (0 for NaN / -inf), D = sum over the candidates (top-k off: over the row).
               The kernel rounds d_j once (u |d_j| absolute, so relative in e_j), calls expf, and divides once:
                   a_j = EXPF_REL + u |d_j| + u                      relative error of e_j / D for an exact D
                   r_D = sum_i q_i (EXPF_REL + u |d_i|) + depth u    relative error of D, q_i = e_i / D,
               depth = n candidates (at most n - 1 additions of non-zero terms, however they are grouped), or ceil(V/256) + 8
               with top-k off (a thread's serial chain, the 6 shuffle levels, the 3 wave sums).  An f32 sum of m stored
               probabilities, in any order, is then within
                   E = sum_j p_j a_j + (r_D + m u) sum_j p_j
               of the float64 sum; r_D is a common factor and drops out wherever two such sums are divided.
  nucleus      candidates:  keep = 1 + the largest j >= 1 whose tail mass T_j = p_j + .. + p_{n-1} exceeds 1 - top_p;
               top-k off:   keep = 1 + the number of leading j >= 1 with 1 - (p_0 + .. + p_{j-1}) > 1 - top_p (one more
               rounding, u).  keep_lo moves every sum by its E against keeping, keep_hi in favour of it.
  draw         the first j with acc_j > u_b * total; acc_j / total is within e_j = cdf_j (E_j / C_j + E_keep / C_keep + 2u) of
               cdf_j = C_j / C_keep (the product u_b * total and the comparison's two operands: 2u).  Pick j is justified iff
               cdf_{j-1} - e_{j-1} <= u_b <= cdf_j + e_j (cdf_{-1} = 0, and the last kept candidate closes the interval).
  A row is determinate when every threshold gap above exceeds TWICE its bound.

Beam step (per batch row): see `BeamStepRef`.
"""
import math

import numpy as np

U = 2.0 ** -24
EXPF_REL = 2.0 * 2.0 ** -23
LOGF_REL = 2.0 * 2.0 ** -23
SAMPLE_CAP = 1024
BEAM_NEG = -1.0e9


# ---- sampler ----------------------------------------------------------------------------------------------------------------
def sampler_scores(row, prev, penalty, temperature):
    """The processed scores as f32 (bit-exact: two IEEE operations).  `prev`: previous token ids, any integers; those
    outside [0, V) are ignored, duplicates count once."""
    x = np.asarray(row, dtype=np.float32)
    V = x.shape[0]
    t, pen = np.float32(temperature), np.float32(penalty)
    with np.errstate(all="ignore"):
        w = x / t
        if pen != np.float32(1.0):
            ids = np.unique(np.asarray([p for p in prev if 0 <= int(p) < V], dtype=np.int64))
            if ids.size:
                xs = x[ids]
                w[ids] = np.where(xs < 0, xs * pen, xs / pen).astype(np.float32) / t
    return w


def sampler_candidates(scores, top_k, cap=SAMPLE_CAP):
    """Token ids of the candidate list in draw order (exact; see the module docstring)."""
    s = np.asarray(scores, dtype=np.float64)
    V = s.shape[0]
    nan = np.isnan(s)
    val = np.where(nan, -np.inf, s)
    order = np.lexsort((np.arange(V), nan, -val))            # value descending, NaN after -inf, token ascending
    k = min(V, cap) if top_k >= V else top_k
    kv, kn = val[order[k - 1]], nan[order[k - 1]]
    ov, on = val[order], nan[order]
    n = int(np.count_nonzero((ov > kv) | ((ov == kv) & (on <= kn))))      # everything not below the k-th
    return order[: min(n, cap)]


class SamplerRef:
    """Float64 distribution of one sampler row with the bounds of the module docstring.  `scores`: the f32 processed scores
    (taken as data), `top_p` / `u`: the f32 values the kernel receives."""

    def __init__(self, scores, top_k, top_p, cap=SAMPLE_CAP):
        s = np.asarray(scores, dtype=np.float64)
        self.V = V = s.shape[0]
        self.full = top_k >= V
        self.cand = cand = sampler_candidates(scores, top_k, cap)
        self.n = n = len(cand)
        top = s[cand[0]]
        with np.errstate(all="ignore"):
            d_row = s - top
            e_row = np.where(np.isfinite(d_row), np.exp(d_row), 0.0)
        d, e = d_row[cand], e_row[cand]
        d = np.where(np.isfinite(d), d, 0.0)                   # e = 0 there: the value of d does not matter
        if self.full:
            D = float(e_row.sum())
            dd = np.where(np.isfinite(d_row), np.abs(d_row), 0.0)
            self.r_D = float((e_row / D * (EXPF_REL + U * dd)).sum()) + (math.ceil(V / 256) + 8) * U
        else:
            D = float(e.sum())
            self.r_D = float((e / D * (EXPF_REL + U * np.abs(d))).sum()) + n * U
        self.p = p = e / D
        self.a = a = EXPF_REL + U * np.abs(d) + U
        self.pa = pa = p * a
        self.thr = float(np.float32(1.0) - np.float32(top_p))  # the kernel's 1.0f - top_p
        self.top_p = float(np.float32(top_p))
        m = np.arange(1, n + 1)
        # prefix sums C_j = p_0 + .. + p_j and suffix sums T_j = p_j + .. + p_{n-1}, with the bounds of their f32 values
        self.C = np.cumsum(p)
        self.EC = np.cumsum(pa) + (self.r_D + m * U) * self.C
        self.T = np.cumsum(p[::-1])[::-1]
        self.ET = np.cumsum(pa[::-1])[::-1] + (self.r_D + m[::-1] * U) * self.T
        self.keep, self.keep_lo, self.keep_hi, self.cut_determinate = self._cut()

    def _cut(self):
        n, thr = self.n, self.thr
        if self.top_p >= 1.0:
            return n, n, n, True
        if self.full:                                          # keeps j >= 1 while 1 - C_{j-1} > thr, stops at the first failure
            rest, e = 1.0 - self.C[:-1], self.EC[:-1] + U
            def lead(mask):
                bad = np.nonzero(~mask)[0]
                return 1 + (int(bad[0]) if bad.size else n - 1)
            keep, lo, hi = lead(rest > thr), lead(rest - e > thr), lead(rest + e > thr)
            gap, e2 = np.abs(rest - thr), 2 * e
        else:                                                  # the largest j >= 1 whose tail mass exceeds thr
            T, e = self.T[1:], self.ET[1:]
            def last(mask):
                good = np.nonzero(mask)[0]
                return 2 + int(good[-1]) if good.size else 1
            keep, lo, hi = last(T > thr), last(T - e > thr), last(T + e > thr)
            gap, e2 = np.abs(T - thr), 2 * e
        return keep, lo, hi, bool(np.all(gap > e2))

    def kept(self, keep=None):
        """(cdf, e_cdf, probs, e_probs) over the first `keep` candidates: cdf_j = C_j / C_keep with the bound of the
        kernel's acc_j / total (+ the rounding of u * total), and the renormalised probabilities with theirs."""
        keep = self.keep if keep is None else keep
        C, pa, p = self.C[:keep], self.pa[:keep], self.p[:keep]
        m = np.arange(1, keep + 1)
        tot = C[-1]
        E = np.cumsum(pa) + m * U * C                          # r_D cancels in every ratio below
        r_tot = E[-1] / tot
        with np.errstate(all="ignore"):
            cdf = C / tot
            e_cdf = cdf * (np.where(C > 0, E / np.where(C > 0, C, 1.0), 0.0) + r_tot + 2 * U)
        jl = int(np.nonzero(p > 0)[0][-1]) if np.any(p > 0) else keep - 1
        e_cdf[jl:] = 0.0                                       # from the last candidate with any mass on, acc IS total (+ 0 is exact)
        cdf[jl:] = 1.0
        probs = p / tot
        return cdf, e_cdf, probs, probs * (self.a[:keep] + r_tot + U)

    def justified_picks(self, u, keep=None):
        """Indices j (into the kept list) that the draw `u` (f32, in [0, 1)) justifies."""
        cdf, e, _, _ = self.kept(keep)
        u = float(np.float32(u))
        lo = np.concatenate([[0.0], cdf[:-1] - e[:-1]])
        hi = cdf + e
        hi[-1] = np.inf
        ok = (lo <= u) & (u <= hi)
        # a candidate without mass never moves acc: it cannot be the first to exceed the target
        ok &= self.p[: len(cdf)] > 0
        return np.nonzero(ok)[0]

    def pick(self, u, keep=None):
        """(the float64 pick, whether twice the bound separates u from every CDF step)."""
        cdf, e, _, _ = self.kept(keep)
        u = float(np.float32(u))
        j = int(np.searchsorted(cdf, u, side="right"))        # first j with cdf_j > u
        j = min(j, len(cdf) - 1)
        inner = cdf < 1.0                                      # the steps before the one that closes the interval
        return j, bool(np.all(np.abs(cdf[inner] - u) > 2 * e[inner]))


# ---- beam step ----------------------------------------------------------------------------------------------------------------
class BeamStepRef:
    """One `icl_beam_step` launch for ONE batch row in float64, driven by the state the launch finds (HF `_beam_search`,
    early_stopping=False; the float32 whole-search restatement is oracle.models.BeamBookkeeping).

    logits  f32 [rows, V] (rows = 1: the K beams share the row; rows = K), NaN = -inf;  m_k = max, d = x - m_k,
            l_k = log sum exp(d), lp = d - l_k;  repetition penalty (step > 0) on the tokens of run_seq[k, :step]:
            lp < 0 ? lp * pen : lp / pen;  a = lp + run_score[k].
    Bound of the kernel's f32 a (first order):
        e_l  = (ceil(V/256) + 8) u + sum_v p_v (EXPF_REL + u |d_v|) + LOGF_REL |l|     the log-sum: the summation depth of a
               thread's chain + the tree, each term's expf and the rounding of its argument, logf
        e_lp = u |d| + u |lp| + e_l                                                    the two subtractions
        penalised: e_lp <- pen' e_lp + u |lp'|,  pen' = pen (lp < 0) or 1 / pen
        e_a  = e_lp + u |a|                                                            the addition of the incoming score
    -inf stays -inf exactly (bound 0).  A continuation that stops runs on at a - 1e9: one more rounding, u |a - 1e9|.
    Finished candidates: s = a / lenpen, lenpen = f32((step + 1) ** length_penalty): e_s = e_a / lenpen + u |s|.

    Bookkeeping as the header states it.  Continuations pushed down by 1e9 (not among the first K, not stopping, or the row is
    closed) never take a finished slot: every a is <= 0 (lp <= 0 and the incoming scores are), so their f32 score is <= -1e9
    by the monotonicity of rounding, every old slot holds >= -1e9, and old slots come first on ties — they are left out of the
    merge here, which changes nothing in exact arithmetic either.

    determinate: every decision below has a float64 gap above twice the larger of the two bounds —
      * neighbours among the best NC + 1 continuations (bit-equal logits of one beam with equal penalty treatment, and -inf
        against -inf, are exact ties in the kernel too and go to the lower beam * V + token);
      * a running continuation against a stopped one among the best K + 1 run values (two of the same kind keep their order
        whatever the rounding: adding -1e9 is monotone);
      * a stopping candidate against an old finished slot among the best K + 1 slot scores (old slots are f32 data, exact;
        two candidates keep their order: the division is monotone);
      * the best running score / lenpen against the worst finished score (only while the row is open).
    """

    def __init__(self, logits, V, K, T, step, eos, length_penalty, rep_pen, run_score, run_seq, fin_score, fin_seq, fin_len,
                 fin_flag, unsat):
        self.V, self.K, self.T, self.step = V, K, T, step
        eos = [int(e) for e in (eos if isinstance(eos, (tuple, list)) else [eos]) if int(e) >= 0]
        self.eos = eos
        self.NC = NC = (3 if len(eos) > 1 else 2) * K
        self.lenpen = lenpen = float(np.float32(float(step + 1) ** float(length_penalty)))
        rep = float(np.float32(rep_pen))
        x = np.asarray(logits, dtype=np.float64)[:, :V]
        if x.shape[0] == 1:
            x = np.repeat(x, K, 0)
        x = np.where(np.isnan(x), -np.inf, x)
        rs = np.asarray(run_score, dtype=np.float64)
        self.old_run = np.asarray(run_seq).copy()
        a = np.empty((K, V))
        e = np.empty((K, V))
        self.pen_mask = np.zeros((K, V), dtype=bool)
        self.x = x
        with np.errstate(all="ignore"):
            for k in range(K):
                m = x[k].max()
                if not m > -np.inf:
                    m = 0.0
                d = x[k] - m
                ex = np.exp(d)
                z = ex.sum()
                l = math.log(z) if z > 0 else -np.inf
                fin = np.isfinite(d)
                da = np.where(fin, np.abs(d), 0.0)
                e_l = ((math.ceil(V / 256) + 8) * U + float((ex / z * (EXPF_REL + U * da)).sum()) + LOGF_REL * abs(l)) if z > 0 else 0.0
                lp = np.where(fin, d - l, -np.inf)
                e_lp = U * da + U * np.abs(np.where(fin, lp, 0.0)) + e_l
                if rep != 1.0 and step > 0:
                    seen = np.unique([t for t in self.old_run[k, :step].tolist() if 0 <= t < V]).astype(np.int64)
                    if seen.size:
                        self.pen_mask[k, seen] = True
                        f = np.where(lp[seen] < 0, rep, 1.0 / rep)
                        lp[seen] = lp[seen] * f
                        e_lp[seen] = e_lp[seen] * f + U * np.abs(np.where(np.isfinite(lp[seen]), lp[seen], 0.0))
                a[k] = lp + rs[k]
                e[k] = np.where(fin, e_lp + U * np.abs(np.where(fin, a[k], 0.0)), 0.0)
        self.a, self.e = a, e
        flat, eflat = a.reshape(-1), e.reshape(-1)
        n_take = min(NC + 1, K * V)
        order = np.lexsort((np.arange(K * V), -flat))[:n_take]
        self.order = order
        self.ci = order[:NC]
        self.cv, self.ce = flat[self.ci], eflat[self.ci]
        last = step + 1 >= T
        self.stops = np.array([last or (int(i) % V) in eos for i in self.ci])
        self.row_open = bool(unsat)
        det = True
        # --- gaps among the best NC + 1 continuations
        for r in range(n_take - 1):
            i, j = int(order[r]), int(order[r + 1])
            vi, vj = flat[i], flat[j]
            if vi == -np.inf and vj == -np.inf:
                continue
            ki, ti, kj, tj = i // V, i % V, j // V, j % V
            if ki == kj and x[ki, ti] == x[kj, tj] and self.pen_mask[ki, ti] == self.pen_mask[kj, tj]:
                continue
            if not (vi - vj) > 2 * max(eflat[i], eflat[j]):
                det = False
        # --- running beams: the K best of a (- 1e9 if it stops), earlier candidate first on ties
        runv = self.cv + np.where(self.stops, BEAM_NEG, 0.0)
        rune = self.ce + np.where(self.stops, U * np.abs(np.where(np.isfinite(runv), runv, 0.0)), 0.0)
        ro = np.lexsort((np.arange(NC), -runv))
        for r in range(min(K, NC - 1)):
            i, j = int(ro[r]), int(ro[r + 1])
            if self.stops[i] != self.stops[j] and not (runv[i] - runv[j]) > 2 * max(rune[i], rune[j]):
                det = False
        self.run_src = ro[:K]
        self.runv, self.rune = runv, rune
        self.run_score = runv[self.run_src]
        self.run_score_e = rune[self.run_src]
        self.next_ids = (self.ci[self.run_src] % V).astype(np.int64)
        self.parent = (self.ci[self.run_src] // V).astype(np.int64)          # beam of the row (the kernel adds b * K)
        self.run_seq = self.old_run[self.parent].copy()
        self.run_seq[:, step] = self.next_ids
        # --- finished slots
        old_s = np.asarray(fin_score, dtype=np.float64)
        ms, me, src = list(old_s), [0.0] * K, list(range(K))
        if self.row_open:
            for j in range(min(K, NC)):
                if self.stops[j]:
                    s = self.cv[j] / lenpen
                    ms.append(s)
                    me.append(self.ce[j] / lenpen + U * abs(s) if np.isfinite(s) else 0.0)
                    src.append(K + j)
        ms, me = np.array(ms), np.array(me)
        fo = np.lexsort((np.arange(len(ms)), -ms))
        for r in range(min(K, len(ms) - 1)):
            i, j = int(fo[r]), int(fo[r + 1])
            if (src[i] < K) != (src[j] < K) and not (ms[i] - ms[j]) > 2 * max(me[i], me[j]):
                det = False
        sel = fo[:K]
        self.fin_src = [src[i] for i in sel]
        self.fin_score, self.fin_score_e = ms[sel], me[sel]
        old_flag, old_len, old_fin = np.asarray(fin_flag), np.asarray(fin_len), np.asarray(fin_seq)
        self.fin_flag = np.array([int(old_flag[s]) if s < K else 1 for s in self.fin_src])
        self.fin_len = np.array([int(old_len[s]) if s < K else step + 1 for s in self.fin_src])
        self.fin_seq = np.empty((K, T), dtype=np.int64)
        for i, s in enumerate(self.fin_src):
            if s < K:
                self.fin_seq[i] = old_fin[s]
            else:
                c = int(self.ci[s - K])
                self.fin_seq[i] = self.old_run[c // V]
                self.fin_seq[i, step] = c % V
        # --- can the best running beam still beat the worst finished hypothesis?
        w = int(np.argmin(self.fin_score))
        worst, worst_e = self.fin_score[w], self.fin_score_e[w]
        best = self.run_score[0] / lenpen
        best_e = self.run_score_e[0] / lenpen + U * abs(best) if np.isfinite(best) else 0.0
        any_ = False
        for i in range(K):
            thr, te = (worst, worst_e) if self.fin_flag[i] else (BEAM_NEG, 0.0)
            any_ = any_ or bool(best > thr)
            if self.row_open and not abs(best - thr) > 2 * max(best_e, te):
                det = False
        self.unsat = int(self.row_open and any_)
        self.determinate = det

    def score_of(self, parent, token):
        """(float64 run value, bound) of continuing beam `parent` with `token`, with the -1e9 of a stopping one."""
        a, e = self.a[parent, token], self.e[parent, token]
        if self.step + 1 >= self.T or token in self.eos:
            a = a + BEAM_NEG
            e = e + U * abs(a) if np.isfinite(a) else 0.0
        return a, e

"""The path kernels of the covariance family (sgdnet_amd/csrc/covariance.hip: cov_path_kernel, cov_group_path_kernel,
cov_wide_path_kernel, cov_wide_group_path_kernel and the cross-validation entries around the same bodies) sweep by sweep,
shared by tests/test_covariance_path_reference.py (CPU), tests/test_gpu_covariance_path_passes.py and
tests/test_gpu_cv_covariance_path_passes.py (GPU): ONE restatement parameterised over (one response | blocks of K) x (all
coordinates | list with screen), in float64 and in long double, the wrong versions of it the checks must reject, a
long-double replay of one sweep with a propagated first-order error bound, and the checks themselves.

The error model is that of tests/setup_reference.py and tests/newton_reference.py (imported): u = 2^-53, one rounding per
operation, a sum of m terms in ANY order errs by at most gamma_m sum|t_i|.  No tolerance in this file comes from what a
device returned.  newton_reference.optimality and single_sweep_reference are restated here rather than called: they take
Newton's (p + 2)^2 moment matrix with an intercept coordinate, one response, all coordinates and a model about u_cur; the
terms of their bounds (conv, drift, local; E_z, E_nu, E_d, E_g) are kept by name and extended to K responses, a list with
screens, a warm start and the rebuild.

Everything starts from what the path kernel was handed, as the probes tap it (a `Model`):
  narrow forms  M, scale, n.  S_jk = M_jk / n / (s_j s_k) and c~_jr = M_(j, p + r) / n / s_j are formed in long double; the
                kernel rounds three times per entry of S and twice per entry of c~: ES = 3 u |S|, Ec = 2 u |c~|
                (newton_reference.model_from_M does the same for H and q).
  wide forms    S, diag S and c~ exactly as tapped (they are the kernel's operands: ES = Ec = 0); the pad rows of S must be 0.

The algorithm (run_path), per lambda, warm-started from the lambda before:
  rebuild   listed: the list becomes {j : w_j. != 0}, ascending.  g = sum_{j in list} S[:, j] w_j. - c~ afresh.
  screen    listed only: every j outside the list gets the update from w_j. = 0; those that would move join; ascending.
  sweep     cyclic (block) coordinate descent over the list (all j when not listed); a move by d does g[k] += S[k, j] d for
            ALL k.  The sweep ends with max|dw| / max|w| <= tol over the coordinates it visited, both maxima of THIS sweep,
            max|w| over the NEW values; all zero counts as converged.  listed: when the rule is met the screen runs again and
            the lambda is done when it adds nothing.  max_iter bounds the list sweeps of one lambda, not of one screen.
  one response:  w_j <- soft(S_jj w_j - g_j, l1) / (S_jj + l2)        (the ridge functor: no threshold), 0 if S_jj + l2 <= 0
  blocks:        z = S_jj w_j. - g_j.,  w_j. <- max(0, 1 - l1 / |z|) z / (S_jj + l2)   (ridge: z / (S_jj + l2)), 0 if |z| = 0

The checks, per job and per lambda (check_outputs, check_replay, check_counts):
  A  exact     1 <= sweeps <= max_iter; unconverged in {0, 1}; unconverged = 1 implies sweeps = max_iter; W_j. = 0.0 where
               S_jj + l2 <= 0; (the callers: equal bytes between widths, the pad of S).
  B  gradient  |G[k] - (S W - c~)[k]| <= rebuild + drift (+ the model's roundings in the narrow forms):
               rebuild  gamma(|list| + 1) (sum_j |S_kj| |w_j| + |c~_k|), w the warm start the rebuild summed over
               drift    2 u sweeps |list| S_k,  S_k = sum_j |S_kj| D + |c~_k|,  D = 2 max(max|w - w_start|, max|w|, max|w_start|)
               (newton_reference, "Inner solve": drift_j).  |list| = p: the list is not returned.
  C  optimum   of a converged lambda, B_jr = conv + drift + local as newton_reference.optimality derives them, here for K
               responses and a warm start:
               conv   (sum_k |S_jk| - |S_jj|) tol max|w|
               local  one response: 8 u (S_j + l1 + (|S_jj| + l2) max|w|), newton_reference's count.
                      blocks: (8 + K + 1 + 2 + 3) u (...): on top of the 8 the K roundings of the fma chain of |z|^2, one of the
                      sqrt, two of 1 - l1 / |z| (the division, the subtraction) and three of group_new_w (the fma of z,
                      the product with the shrink, the division).
               one response: |g_j| <= l1 + B_j where w_j = 0, |g_j + l2 w_j + l1 sign w_j| <= B_j elsewhere (ridge: l1 = 0 in
               both).  blocks: |g_j.| <= l1 + |B_j.| for a zero block, |g_j. + l2 w_j. + l1 w_j. / |w_j.|| <= |B_j.| elsewhere.
               g = S W - c~ in long double: the condition is on the returned W itself.
  D  replay    max_iter = 1 on REPLAY_RATIOS (three decreasing lambdas, then a larger one) with tol = REPLAY_TOL.  For
               every lambda the long-double reference starts from the device's own W of the lambda before (zeros first),
               rebuilds, (screens,) sweeps once (and screens again) and propagates a first-order bound, times 1.01 for
               the second-order terms, with the recurrences of newton_reference.single_sweep_reference:
                 E_g after the rebuild = gamma(|list| + 1)(sum_j |S_kj w_j| + |c~_k|) + sum_j ES_kj |w_j| + Ec_k
                 E_z = |w_j| ES_jj + E_g_j + u (|S_jj w_j| + |z|),   E_den = ES_jj + u den
                 one response:  E_nw = (E_z + u |soft z| + |nw| E_den) / (den - E_den) + u |nw|
                 blocks:  E_zz = sum_r 2 |z_r| E_z_r + gamma(K) |z|^2,  E_|z| = E_zz / (2 |z|) + u |z|,
                          q = l1 / |z|: E_q = q E_|z| / (|z| - E_|z|) + u q,   E_shrink = E_q + u shrink,
                          E_nw_r = (|z_r| E_shrink + shrink E_z_r + 2 u |shrink z_r| + |nw_r| E_den) / (den - E_den) + u |nw_r|
                 E_d = E_nw + u |d|,   E_g_k += |S_kj| E_d + |d| ES_kj + u |S_kj d| + u (|g_k| + E_g_k)
               Required: |W - ref| <= E, |G - ref_g| <= E_g, sweeps = 1, unconverged as the reference's control flow has it
               (listed: 1 unless the sweep met tol and the second screen added nothing).
  E  counts    for (tol, max_iter) in COUNT_SETTINGS: sweeps and unconverged equal those of the float64 restatement.

Preconditions of D and E, asserted by the reference on the inputs ("input too close to a decision"), never skipped:
  decisions  the long-double value a screen or a threshold compares (|g_j|, |z| against l1; S_jj + l2 against 0) is farther
             from its threshold than 2^20 times its bound (D: the propagated one; E: the roundings g_j has collected so far,
             Guard.bound), or sits on it exactly with a bound of 0 (a constant column: S_jj = c~_j = 0).
  stops      at the end of every sweep of the long-double restatement |ratio / tol - 1| > 1e-6.
  length     max_iter = 1000: the long-double restatement converges in at most 200 sweeps per lambda."""
from types import SimpleNamespace

import numpy as np

from newton_reference import pair_sum
from setup_reference import LD, U, Val, gamma

REPLAY_RATIOS = (0.6, 0.35, 0.2, 0.3)     # of the lambda at which the first coordinate moves: three decreasing, one larger
REPLAY_TOL = 0.5                          # one sweep from a warm start meets it at some lambdas and misses it at others
COUNT_SETTINGS = [(1e-7, 2), (1e-7, 5), (1e-3, 1000), (1e-7, 1000)]
DECISION_FACTOR = LD(2.0) ** 20
STOP_MARGIN = 1e-6
LONGEST = 200
COV_MAX_FEATURES, WCOV_MAX_FEATURES = 198, 4531


class Precondition(AssertionError):
    """an input of the test is too close to a decision of the algorithm: choose another input, never a tolerance"""


def _too_close(what):
    raise Precondition(f"input too close to a decision: {what}")


# ---------------------------------------------------------------------------------------------------------------
# the model: what the path kernel was handed
# ---------------------------------------------------------------------------------------------------------------

class Model:
    """S (p x p, symmetric; float64 as tapped, or long double from M), diag S, c~ (p x K) and the relative roundings of the
    kernel's own S and c~ against them"""

    def __init__(self, S, diag, c, rel_S, rel_c):
        self.S, self.diag, self.c, self.rel_S, self.rel_c = S, diag, c, LD(rel_S), LD(rel_c)
        self.p, self.K = c.shape
        self._rows = None

    def col(self, j, F):
        return self.S[:, j].astype(F)

    def abs_rows(self):
        """sum_j |S_kj|, long double (summed in S's own type: p more roundings, covered by the 1 + gamma_p below)"""
        if self._rows is None:
            self._rows = np.abs(self.S).sum(axis=1).astype(LD) * (1 + gamma(self.p + 1))
        return self._rows

    def times(self, w):
        """S w in long double over the non-zero rows of w (p x K)"""
        w = np.asarray(w, dtype=LD)
        out, mag = np.zeros((self.p, self.K), dtype=LD), np.zeros((self.p, self.K), dtype=LD)
        for j in np.flatnonzero((w != 0).any(axis=1)):
            t = self.col(j, LD)[:, None] * w[j][None, :]
            out += t
            mag += np.abs(t)
        return out, mag


def narrow_model(M, scale, n, K, F=LD):
    """cov_path_kernel's / cov_group_path_kernel's prologue from the upper triangle of M (rows j < p), in the kernel's order of
    operations: M / n / (s_j s_k), M / n / s_j"""
    M = np.asarray(M)
    p = M.shape[1] - K
    s = np.asarray(scale, dtype=F)
    Mu = np.asarray(M[:p, :p], dtype=F)
    Mu = np.triu(Mu) + np.triu(Mu, 1).T
    S = Mu / F(n) / np.outer(s, s)
    c = np.asarray(M[:p, p:p + K], dtype=F) / F(n) / s[:, None]
    exact = F is LD
    return Model(S, np.diag(S).copy(), c, 3 * U if exact else 0, 2 * U if exact else 0)


def wide_model(S, Sd, ct):
    """cov_wide_path_kernel's operands as tapped: S p x ld, row j = column j, the pad k >= p (check_pad)"""
    S = np.asarray(S, dtype=np.float64)
    p = S.shape[0]
    return Model(S[:, :p].T, np.asarray(Sd, dtype=np.float64), np.asarray(ct, dtype=np.float64).reshape(p, -1), 0, 0)


def check_pad(S):
    S = np.asarray(S)
    p = S.shape[-2]
    assert np.all(S[..., p:] == 0.0) and not np.any(np.signbit(S[..., p:])), "A: the pad entries of S are not 0.0"


# ---------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------

def _fma(a, b, c):
    """a b + c with one rounding to float64 (through long double: the product keeps 64 bits)"""
    return (np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD) + np.asarray(c, dtype=LD)).astype(np.float64)


def _rebuild(model, w, live, F, order):
    """sum_{j in live} S[:, j] w_j. - c~.  order: "sequential", "pairwise", or "kernel" (j ascending, a fused multiply-add
    per term: the wide kernels request four columns at a time and add them in this order)"""
    p, K = model.p, model.K
    c = model.c.astype(F)
    if len(live) == 0:
        return -c
    if F is LD or order == "sequential":
        g = np.zeros((p, K), dtype=F)
        for j in live:
            g = g + model.col(j, F)[:, None] * w[j][None, :]
        return g - c
    if order == "kernel":
        g = np.zeros((p, K))
        for j in live:
            g = _fma(model.col(j, F)[:, None], w[j][None, :], g)
        return g - c
    terms = np.stack([model.col(j, F)[:, None] * w[j][None, :] for j in live])
    return {"pairwise": pair_sum}[order](terms) - c


def _soft(z, l1):
    return z - l1 if z > l1 else (z + l1 if z < -l1 else z * 0)


class Guard:
    """the preconditions of E, collected by the long-double restatement: every decision against bound(), every stop.
    bound() is first order in g_j's own roundings: gamma(|list| + 1)(sum_{k in list} |S_jk| max|w| + |c~_j|) from the rebuild,
    u (|S_jk d| + |g_j|) for every move since (the actual magnitudes of the long-double run), and the update's own
    (8 + K + 6) u (|S_jj w_j| + |g_j| + l1).  What those errors do to LATER moves is not followed (that recurrence doubles per
    move where columns are correlated and bounds nothing after a few sweeps): the factor 2^20 is the room for it."""

    def __init__(self, model, what):
        self.model, self.absc, self.what = model, np.abs(model.c).astype(LD), what
        self.p, self.K = model.p, model.K
        self.Eg = np.zeros((self.p, self.K), dtype=LD)
        self.closest_decision, self.closest_stop, self.longest = np.inf, np.inf, 0

    def rebuilt(self, live, w):
        rows = np.abs(self.model.S[:, live]).sum(axis=1).astype(LD) * (1 + gamma(len(live) + 1))
        self.Eg = gamma(len(live) + 1) * (rows[:, None] * LD(np.abs(w).max()) + self.absc)

    def moved(self, step, g):
        self.Eg = self.Eg + U * (np.abs(step) + np.abs(g))

    def bound(self, j, l1, sjj, wj, gj):
        return self.Eg[j].sum() + (8 + self.K + 6) * U * self.K * (abs(sjj) * np.abs(wj).max() + np.abs(gj).max() + l1)

    def decision(self, value, threshold, bound, kind, j):
        margin = abs(LD(value) - LD(threshold))
        if margin == 0 and bound == 0:
            return
        if bound > 0:
            self.closest_decision = min(self.closest_decision, float(margin / bound))
        if not margin > DECISION_FACTOR * bound:
            _too_close(f"{self.what}: {kind} of coordinate {j}: {float(value):.17g} against {float(threshold):.17g}, bound {float(bound):.3e}")

    def stop(self, ratio, tol, lam, sweep):
        d = abs(float(ratio) / tol - 1)
        self.closest_stop = min(self.closest_stop, d)
        if not d > STOP_MARGIN:
            _too_close(f"{self.what}: the stopping rule of sweep {sweep} of lambda {lam}: ratio {float(ratio):.17g}, tol {tol}")


def run_path(model, l2s, l1s, ridge, tol, max_iter, *, blocks, listed, F=np.float64, order="kernel", wrong=None, guard=None):
    """The path kernel restated (module docstring).  F: np.float64 or LD.  order: the rebuild's summation order.  wrong: one of
    MUTANTS.  guard: a Guard that asserts the preconditions of E (F = LD).  Returns W, G (L, p, K), sweeps, unconverged (L),
    screens (L), lists (L: the list's final size)."""
    p, K = model.p, model.K
    diag = model.diag.astype(F)
    L = len(l2s)
    w = np.zeros((p, K), dtype=F)
    W, G = np.zeros((L, p, K), dtype=F), np.zeros((L, p, K), dtype=F)
    n_sweeps, unconverged, n_screens, lists = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64)
    change = size = F(0)

    def update(j, l1, l2, decide=None):
        """the new w_j. from the stored w_j. and g_j."""
        sjj = diag[j]
        den = sjj if wrong == "no_l2_in_denominator" else sjj + l2
        if decide:
            decide(sjj + l2, 0, model.rel_S * abs(sjj) + U * abs(sjj + l2), "S_jj + l2 against 0", j)
        z = sjj * w[j] - g[j]
        thresholded = (not ridge or wrong == "ridge_thresholded") and wrong != "lasso_unthresholded"
        if not blocks:
            z0 = z[0]
            if decide and thresholded and den > 0:
                decide(abs(z0), l1, guard.bound(j, l1, sjj, w[j], g[j]), "|z| against l1", j)
            nw = _soft(z0, l1) if thresholded else z0
            return np.array([nw / den if den > 0 else F(0)], dtype=F)
        zs = z[1:] if wrong == "group_norm_skips_response_0" else z
        if wrong == "group_shrink_from_w":
            zs = w[j]
        nz = np.sqrt((zs * zs).sum())
        if decide and thresholded and den > 0:
            decide(nz, l1, guard.bound(j, l1, sjj, w[j], g[j]), "|z| against l1", j)
        shrink = F(1)
        if thresholded:
            shrink = 1 - l1 / nz if nz > l1 else F(0)
        if not nz > 0 or not den > 0:
            shrink = F(0)
        return shrink * z / (den if den > 0 else F(1))

    for l in range(L):
        l2, l1 = F(l2s[l]), F(l1s[l])
        if wrong == "warm_start_dropped":
            w[:] = 0
        in_list = (w != 0).any(axis=1) if listed else np.ones(p, dtype=bool)
        live = np.flatnonzero(in_list)
        g = _rebuild(model, w, live, F, order)
        if guard:
            guard.rebuilt(live, w)
        decide = guard.decision if guard else None
        sweeps, screens, converged = 0, 0, False

        def sweep(live):
            nonlocal w, g, change, size
            if wrong != "max_not_reset":
                change = size = F(0)
            visit = live[::-1] if wrong == "list_descending" else live
            for j in visit:
                nw = update(j, l1, l2, decide)
                d = nw - w[j]
                change = max(change, np.abs(d).max())
                size = max(size, np.abs(w[j]).max() if wrong == "size_before_update" else np.abs(nw).max())
                if np.any(d != 0):
                    w[j] = nw
                    col = model.col(j, F)
                    if F is LD or not (listed or blocks):
                        step = col[:, None] * d[None, :]         # cov_path_kernel: g[k] += S[k, j] * d, no fused multiply-add
                        new_g = g + step
                    else:
                        new_g = _fma(col[:, None], d[None, :], g)
                    if wrong == "tail_not_moved" and p % 2 == 1:
                        new_g[p - 1] = g[p - 1]
                    if wrong == "row_j_not_moved":
                        new_g[j] = g[j]
                    g = new_g
                    if guard:
                        guard.moved(col[:, None] * d[None, :], g)
            if wrong == "absolute_change":
                return bool(change <= tol)
            if guard and size != 0:
                guard.stop(change / size, tol, l, sweeps + 1)
            return bool((size == 0 and change == 0) or (size != 0 and change / size <= tol))

        if not listed:
            while sweeps < max_iter and not converged:
                converged = sweep(live)
                sweeps += 1
        else:
            while True:
                added = np.zeros(p, dtype=bool)
                for j in np.flatnonzero(~in_list):
                    added[j] = np.any(update(j, l1, l2, decide) != 0)
                screens += 1
                if wrong == "sweeps_count_screens":
                    sweeps += 1
                if screens > 1 and (not added.any() or wrong == "no_second_screen"):
                    converged = True
                    break
                in_list |= added
                live = np.flatnonzero(in_list)
                met, budget = False, 0
                while (budget if wrong == "max_iter_per_screen" else sweeps) < max_iter and not met:
                    met = sweep(live)
                    sweeps += 1
                    budget += 1
                if not met:
                    break
        W[l], G[l] = w, g
        n_sweeps[l], unconverged[l], n_screens[l], lists[l] = sweeps, 0 if converged else 1, screens, len(live)
        if guard:
            guard.longest = max(guard.longest, sweeps)
    return SimpleNamespace(W=W, G=G, sweeps=n_sweeps, unconverged=unconverged, screens=n_screens, lists=lists)


MUTANTS = ["no_l2_in_denominator", "ridge_thresholded", "lasso_unthresholded", "max_not_reset", "size_before_update", "absolute_change",
           "sweeps_count_screens", "max_iter_per_screen", "no_second_screen", "warm_start_dropped", "list_descending", "tail_not_moved",
           "row_j_not_moved", "group_shrink_from_w", "group_norm_skips_response_0"]
CV_MUTANTS = ["set_is_job_div_n_sets", "penalties_of_job_0"]


def run_cv(models, pen_a, pen_b, ridge, tol, max_iter, *, blocks, listed, wrong=None, **kw):
    """The job arithmetic of the cross-validation launches: job = mix * n_sets + set, its training set is job % n_sets, its
    penalties, functor and outputs are the job's own.  models: one per training set; pen_a, pen_b (A, G, L); ridge (A, G).
    Returns the fields of run_path with the leading axes (A, G)."""
    A, G, L = pen_a.shape
    pa, pb, rj = pen_a.reshape(A * G, L), pen_b.reshape(A * G, L), np.asarray(ridge).reshape(A * G)
    outs = []
    for job in range(A * G):
        s = job // G if wrong == "set_is_job_div_n_sets" else job % G
        pj = 0 if wrong == "penalties_of_job_0" else job
        outs.append(run_path(models[s], pa[pj], pb[pj], bool(rj[pj]), tol, max_iter, blocks=blocks, listed=listed, **kw))
    return SimpleNamespace(**{k: np.stack([getattr(o, k) for o in outs]).reshape((A, G) + getattr(outs[0], k).shape)
                              for k in ("W", "G", "sweeps", "unconverged")})


def job_of(o, a, t):
    """job (a, t) of the fields of a cross-validation as a single fit's"""
    return SimpleNamespace(W=o.W[a, t], G=o.G[a, t], sweeps=o.sweeps[a, t], unconverged=o.unconverged[a, t])


# ---------------------------------------------------------------------------------------------------------------
# checks A, B, C
# ---------------------------------------------------------------------------------------------------------------

def check_outputs(o, model, l2s, l1s, ridge, tol, max_iter, *, blocks, what, optimum=True, report=None):
    """A, B and (optimum) C on the fields W, G, sweeps, unconverged of one path against the long-double model"""
    p, K = model.p, model.K
    W, G = np.asarray(o.W, dtype=LD).reshape(-1, p, K), np.asarray(o.G, dtype=LD).reshape(-1, p, K)
    sweeps, unconv = np.asarray(o.sweeps).reshape(-1), np.asarray(o.unconverged).reshape(-1)
    L = len(l2s)
    assert W.shape[0] == L and sweeps.shape == (L,) and unconv.shape == (L,), f"{what}: shapes"
    assert not np.any(np.isnan(W)) and not np.any(np.isnan(G)), f"{what}: A: NaN"
    assert np.all((sweeps >= 1) & (sweeps <= max_iter)), f"{what}: A: sweeps {sweeps} outside 1 .. {max_iter}"
    assert np.all((unconv == 0) | (unconv == 1)), f"{what}: A: unconverged {unconv}"
    assert np.all(sweeps[unconv == 1] == max_iter), f"{what}: A: unconverged before max_iter: sweeps {sweeps}, flags {unconv}"
    rows, diag = model.abs_rows(), model.diag.astype(LD)
    c = model.c.astype(LD)
    worst_b = worst_c = 0.0
    mag = np.zeros((p, K), dtype=LD)
    for l in range(L):
        l2, l1 = LD(l2s[l]), LD(0 if ridge else l1s[l])
        w, w0 = W[l], (W[l - 1] if l else np.zeros((p, K), dtype=LD))
        dead = diag + l2 <= 0
        assert np.all(W[l][dead] == 0.0), f"{what}: A: lambda {l}: a coordinate with S_jj + l2 <= 0 is not 0.0"
        mag0 = mag                                   # sum_j |S_kj w_j| at the warm start: what the rebuild added
        Sw, mag = model.times(w)
        g = Sw - c
        wmax = np.abs(w).max()
        D = 2 * max(np.abs(w - w0).max(), wmax, np.abs(w0).max())
        Sk = (rows * D)[:, None] + np.abs(c)
        drift = 2 * U * LD(int(sweeps[l])) * p * Sk
        bound_b = gamma(p + 1) * (mag0 + np.abs(c)) + drift + model.rel_S * mag + model.rel_c * np.abs(c)
        err = np.abs(G[l] - g)
        k = np.unravel_index(np.argmax(err - bound_b), err.shape)
        worst_b = max(worst_b, float((err / np.where(bound_b > 0, bound_b, 1)).max()))
        assert np.all(err <= bound_b), f"{what}: B: lambda {l}: G{tuple(int(i) for i in k)} is off the full gradient by {float(err[k]):.3e}, bound {float(bound_b[k]):.3e}"
        if not optimum or unconv[l]:
            continue
        conv = ((rows - np.abs(diag)) * LD(tol) * wmax)[:, None]
        count = 8 + (K + 1 + 2 + 3 if blocks else 0)
        local = count * U * (Sk + l1 + ((np.abs(diag) + l2) * wmax)[:, None])
        Bj = conv + drift + local + model.rel_S * mag + model.rel_c * np.abs(c)
        if blocks:
            nw = np.sqrt((w * w).sum(axis=1))
            zero = nw == 0
            with np.errstate(divide="ignore", invalid="ignore"):
                direction = np.where(zero[:, None], 0, w / np.where(zero, 1, nw)[:, None])
            res = np.where(zero, np.maximum(np.sqrt((g * g).sum(axis=1)) - l1, 0), np.sqrt(((g + l2 * w + l1 * direction) ** 2).sum(axis=1)))
            Bn = np.sqrt((Bj * Bj).sum(axis=1))
        else:
            res = np.where(w == 0, np.maximum(np.abs(g) - l1, 0), np.abs(g + l2 * w + l1 * np.sign(w)))[:, 0]
            Bn = Bj[:, 0]
        res, Bn = res[~dead], Bn[~dead]
        if res.size:
            k = int(np.argmax(res - Bn))
            worst_c = max(worst_c, float((res / Bn).max()))
            assert np.all(res <= Bn), f"{what}: C: lambda {l}: coordinate {np.flatnonzero(~dead)[k]} misses optimality by {float(res[k]):.3e}, bound {float(Bn[k]):.3e}"
    print(f"{what}: B: largest |G - (S W - c)| / bound {worst_b:.3e}; C: largest residual / bound {worst_c:.3e}; sweeps {sweeps.tolist()}")
    if report is not None:
        report.append((what, "B", worst_b))
        if optimum:
            report.append((what, "C", worst_c))


# ---------------------------------------------------------------------------------------------------------------
# check D: one sweep in long double, error propagated
# ---------------------------------------------------------------------------------------------------------------

def replay_reference(model, W_dev, l2s, l1s, ridge, tol, *, blocks, listed, what):
    """For every lambda: Val W, Val G after rebuild, (screen,) one sweep (and the second screen) from the device's own W of the
    lambda before, and the unconverged flag the control flow gives.  Asserts the preconditions (module docstring)."""
    p, K = model.p, model.K
    diag, c = model.diag.astype(LD), model.c.astype(LD)
    Ed_all = model.rel_S * np.abs(diag)
    Ec = model.rel_c * np.abs(c)
    L = len(l2s)
    W_dev = np.asarray(W_dev, dtype=LD).reshape(L, p, K)
    out = []
    closest = np.inf

    def decision(value, threshold, bound, kind, j, l):
        nonlocal closest
        margin = abs(value - threshold)
        if margin == 0 and bound == 0:
            return
        if bound > 0:
            closest = min(closest, float(margin / bound))
        if not margin > DECISION_FACTOR * bound:
            _too_close(f"{what}: lambda {l}: {kind} of coordinate {j}: {float(value):.17g} against {float(threshold):.17g}, bound {float(bound):.3e}")

    for l in range(L):
        l2, l1 = LD(l2s[l]), LD(l1s[l])
        w = W_dev[l - 1].copy() if l else np.zeros((p, K), dtype=LD)
        Ew = np.zeros((p, K), dtype=LD)
        in_list = (w != 0).any(axis=1) if listed else np.ones(p, dtype=bool)
        live = np.flatnonzero(in_list)
        g, mag, ES_w = -c.copy(), np.abs(c).copy(), np.zeros((p, K), dtype=LD)
        for j in live:
            t = model.col(j, LD)[:, None] * w[j][None, :]
            g, mag, ES_w = g + t, mag + np.abs(t), ES_w + model.rel_S * np.abs(t)
        Eg = gamma(len(live) + 1) * mag + ES_w + Ec

        def update(j, screening):
            """(nw, E_nw) of coordinate j from w[j], g[j] and their bounds; the decisions are asserted"""
            sjj, Esjj = diag[j], Ed_all[j]
            den = sjj + l2
            Eden = Esjj + U * abs(den)
            decision(den, LD(0), Eden, "S_jj + l2 against 0", j, l)
            z = sjj * w[j] - g[j]
            Ez = np.abs(w[j]) * Esjj + Eg[j] + U * (np.abs(sjj * w[j]) + np.abs(z))
            if not den > 0:
                return np.zeros(K, dtype=LD), np.zeros(K, dtype=LD)
            if not blocks:
                z0, Ez0 = z[0], Ez[0]
                if not ridge:
                    decision(abs(z0), l1, Ez0, "|z| against l1", j, l)
                elif screening:
                    decision(abs(z0), LD(0), Ez0, "z against 0 (ridge)", j, l)
                sz = z0 if ridge else _soft(z0, l1)
                nw = sz / den
                Enw = (Ez0 + U * abs(sz) + abs(nw) * Eden) / (den - Eden) + U * abs(nw)
                if sz == 0:
                    Enw = LD(0)                      # decided with a margin: the kernel's value is exactly 0 too
                return np.array([nw]), np.array([Enw])
            zz = (z * z).sum()
            nz = np.sqrt(zz)
            if nz == 0 and not np.any(Ez > 0):
                return np.zeros(K, dtype=LD), np.zeros(K, dtype=LD)
            Ezz = (2 * np.abs(z) * Ez).sum() + gamma(K) * zz
            Enz = Ezz / (2 * nz) + U * nz if nz > 0 else np.sqrt(Ezz)
            if not ridge or screening:
                decision(nz, LD(0) if ridge else l1, Enz, "|z| against l1", j, l)
            if ridge:
                shrink, Eshrink = LD(1), LD(0)
            elif nz > l1:
                q = l1 / nz
                Eq = q * Enz / (nz - Enz) + U * q
                shrink = 1 - q
                Eshrink = Eq + U * shrink
            else:
                return np.zeros(K, dtype=LD), np.zeros(K, dtype=LD)
            nw = shrink * z / den
            Enw = (np.abs(z) * Eshrink + shrink * Ez + 2 * U * np.abs(shrink * z) + np.abs(nw) * Eden) / (den - Eden) + U * np.abs(nw)
            return nw, Enw

        def screen():
            added = np.zeros(p, dtype=bool)
            for j in np.flatnonzero(~in_list):
                added[j] = np.any(update(j, True)[0] != 0)
            return added

        if listed:
            in_list |= screen()
            live = np.flatnonzero(in_list)
        change = size = LD(0)
        for j in live:
            nw, Enw = update(j, False)
            d = nw - w[j]
            Edj = Enw + U * np.abs(d)
            change, size = max(change, np.abs(d).max()), max(size, np.abs(nw).max())
            if np.any(d != 0):
                w[j], Ew[j] = nw, Enw
                col = np.abs(model.col(j, LD))
                upd = model.col(j, LD)[:, None] * d[None, :]
                g = g + upd
                Eg = Eg + col[:, None] * Edj[None, :] + model.rel_S * np.abs(upd) + U * np.abs(upd) + U * (np.abs(g) + Eg)
        if size != 0:
            if not abs(float(change / size) / tol - 1) > STOP_MARGIN:
                _too_close(f"{what}: lambda {l}: the stopping rule: ratio {float(change / size):.17g}, tol {tol}")
        met = bool((size == 0 and change == 0) or (size != 0 and change / size <= tol))
        if listed and met:
            met = not screen().any()
        out.append(SimpleNamespace(W=Val(w, LD(1.01) * Ew), G=Val(g, LD(1.01) * Eg), unconverged=0 if met else 1))
    return out, closest


def check_replay(o, model, l2s, l1s, ridge, tol, *, blocks, listed, what, report=None, model64=None):
    """D on the fields of a path run with max_iter = 1.  model64: also hold W and G to the float64 restatement's one-sweep path,
    within 2 E (both are within E of the long-double replay)."""
    p, K = model.p, model.K
    L = len(l2s)
    W, G = np.asarray(o.W).reshape(L, p, K), np.asarray(o.G).reshape(L, p, K)
    ref, closest = replay_reference(model, W, l2s, l1s, ridge, tol, blocks=blocks, listed=listed, what=what)
    sweeps, unconv = np.asarray(o.sweeps).reshape(-1), np.asarray(o.unconverged).reshape(-1)
    worst = 0.0
    for l in range(L):
        assert sweeps[l] == 1, f"{what}: D: lambda {l}: {sweeps[l]} sweeps with max_iter = 1"
        for got, want, name in ((W[l], ref[l].W, "W"), (G[l], ref[l].G, "G")):
            err = np.abs(np.asarray(got, dtype=LD) - want.v)
            k = np.unravel_index(np.argmax(err - want.e), err.shape)
            if np.any(want.e > 0):
                worst = max(worst, float((err[want.e > 0] / want.e[want.e > 0]).max()))
            assert np.all(err <= want.e), f"{what}: D: lambda {l}: {name}{tuple(int(i) for i in k)} differs from the replayed sweep by {float(err[k]):.3e}, bound {float(want.e[k]):.3e}"
        assert unconv[l] == ref[l].unconverged, f"{what}: D: lambda {l}: unconverged {unconv[l]}, the replayed control flow says {ref[l].unconverged}"
    if model64 is not None:
        f64 = run_path(model64, l2s, l1s, ridge, tol, 1, blocks=blocks, listed=listed, order="kernel" if listed else "sequential")
        for l in range(L):
            start_same = l == 0 or np.array_equal(W[l - 1], f64.W[l - 1])
            for got, want, bound, name in ((W[l], f64.W[l], ref[l].W.e, "W"), (G[l], f64.G[l], ref[l].G.e, "G")):
                if start_same:               # (from another start the two sweeps are not one sweep apart)
                    assert np.all(np.abs(np.asarray(got, dtype=LD) - want) <= 2 * bound), f"{what}: D: lambda {l}: {name} against the float64 restatement"
    print(f"{what}: D: largest error / propagated bound {worst:.3e}; closest decision {closest:.3e} bounds away; flags {unconv.tolist()}")
    if report is not None:
        report.append((what, "D", worst))


# ---------------------------------------------------------------------------------------------------------------
# check E and its preconditions
# ---------------------------------------------------------------------------------------------------------------

def check_counts(run_device, model64, model_ld, l2s, l1s, ridge, *, blocks, listed, what, order=None, settings=COUNT_SETTINGS, report=None,
                 cache=None):
    """E.  run_device(tol, max_iter) -> the fields of a path; model64: what the kernel computes with, in float64 (narrow:
    narrow_model(..., F=np.float64); wide: the tapped model itself); model_ld: the long-double model the preconditions are
    asserted on.  Returns the device's fields per setting."""
    order = order or ("kernel" if listed else "sequential")
    outs = {}
    for tol, max_iter in settings:
        if cache is not None and (tol, max_iter) in cache:
            guard, f64 = cache[(tol, max_iter)]
        else:
            guard = Guard(model_ld, f"{what} (tol {tol}, max_iter {max_iter})")
            ld = run_path(model_ld, l2s, l1s, ridge, tol, max_iter, blocks=blocks, listed=listed, F=LD, guard=guard)
            if max_iter == 1000 and not (guard.longest <= LONGEST and not ld.unconverged.any()):
                _too_close(f"{what}: the long-double restatement takes {guard.longest} sweeps at tol {tol} (at most {LONGEST})")
            f64 = run_path(model64, l2s, l1s, ridge, tol, max_iter, blocks=blocks, listed=listed, order=order)
            f64.screens_ld = ld.screens
            if cache is not None:
                cache[(tol, max_iter)] = (guard, f64)
        o = run_device(tol, max_iter)
        sw, un = np.asarray(o.sweeps).reshape(-1), np.asarray(o.unconverged).reshape(-1)
        print(f"{what}: E: tol {tol}, max_iter {max_iter}: sweeps {sw.tolist()}, unconverged {un.tolist()}; closest stop {guard.closest_stop:.3e}, "
              f"closest decision {guard.closest_decision:.3e} bounds away")
        assert np.array_equal(sw, f64.sweeps), f"{what}: E: tol {tol}, max_iter {max_iter}: sweeps {sw.tolist()}, the restatement takes {f64.sweeps.tolist()}"
        assert np.array_equal(un, f64.unconverged), f"{what}: E: tol {tol}, max_iter {max_iter}: unconverged {un.tolist()}, the restatement has {f64.unconverged.tolist()}"
        outs[(tol, max_iter)] = o
        if report is not None:
            report.append((what, f"E tol {tol} max_iter {max_iter}", sw.tolist()))
    return outs


def same_bytes(a, b, what):
    for name in ("W", "G", "sweeps", "unconverged"):
        x, y = np.ascontiguousarray(getattr(a, name)), np.ascontiguousarray(getattr(b, name))
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: A: {name} differs between the two runs"


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------

def mcov_max_features(K):
    p = 1
    while (p + 1) * (p + 2) // 2 + 3 * (p + 1) * K <= 20480:
        p += 1
    return p


def wmcov_max_features(K):
    import wmcovariance_reference as wm
    return wm.max_features(K)


def make_case(form, n, p, K, mix, *, seed=0, constant=None, sparse=False, ratios=REPLAY_RATIOS, count_ratios=None, xy=None):
    """One fit's inputs as the probe takes them.  form: "cov", "mcov", "wcov", "wmcov".  x dense with columns of different
    scales and a common factor (so that S is not nearly diagonal), y = x B + noise, centred (and, one response, scaled) as
    the driver hands it over; scale = the columns' sd.  constant: a column set to one value (S_jj = c~_j = 0).  The lambdas are
    ratios of the one at which the first coordinate moves (the ridge functor: 5 max(1, p / n) times that, so that the l2 term is of
    the order of S's largest eigenvalue and the sweeps of p coupled coordinates end within LONGEST): lam for check D, lam_counts (the same unless count_ratios says otherwise) for check E."""
    import scipy.sparse as sp
    rng = np.random.default_rng(100000 * seed + 1000 * n + 7 * p + K)
    if xy is None:
        x = (rng.standard_normal((n, p)) + 0.5 * rng.standard_normal((n, 1))) * rng.uniform(0.5, 3.0, p) + rng.uniform(-1.0, 1.0, p)
        B = rng.standard_normal((p, K)) * (rng.random(p) < min(1.0, 8.0 / p))[:, None]
        B[0] = rng.standard_normal(K) + 1.5
        y = x @ B + 0.5 * rng.standard_normal((n, K))
    else:
        x, y = xy
        y = np.asarray(y, dtype=float).reshape(n, K)
    if sparse:
        keep = rng.random((n, p)) < 0.4
        keep[0, :] = True
        x = x * keep
    if constant is not None:
        x[:, constant] = 1.25
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    scale = np.where(var == 0, 1.0, np.sqrt(var))
    y = y - y.mean(axis=0)
    if form in ("cov", "wcov"):
        y = y / y.std(axis=0)
    c = ((x - mean) / scale).T @ y / n
    top = np.sqrt((c * c).sum(axis=1)).max()
    top = top / mix if mix > 0 else 5.0 * max(1.0, p / n) * top
    lam, lam_counts = top * np.asarray(ratios), top * np.asarray(ratios if count_ratios is None else count_ratios)
    return SimpleNamespace(form=form, n=n, p=p, K=K, mix=mix, x=sp.csc_matrix(x) if sparse else x, xd=x, y=y if K > 1 or form in ("mcov", "wmcov") else y[:, 0],
                           scale=scale, lam=lam, wide=form in ("wcov", "wmcov"), multi=form in ("mcov", "wmcov"), blocks=form in ("mcov", "wmcov"),
                           listed=form in ("wcov", "wmcov"), ridge=mix == 0.0, l2=(1.0 - mix) * lam, l1=mix * lam, lam_counts=lam_counts,
                           l2_counts=(1.0 - mix) * lam_counts, l1_counts=mix * lam_counts,
                           name=f"{form} n{n} p{p} K{K} mix{mix}" + (f" constant{constant}" if constant is not None else "") + (" sparse" if sparse else ""))


def host_models(case):
    """what the moments and scale stages hand the path kernel, formed on the host in float64 (the device's differ by
    roundings only): (model64, model_ld)"""
    xc = case.xd - case.xd.mean(axis=0)
    y = np.asarray(case.y, dtype=float).reshape(case.n, case.K)
    A = np.concatenate([xc, y], axis=1)
    M = A.T @ A
    const = np.flatnonzero((xc == 0).all(axis=0))
    M[const, :], M[:, const] = 0.0, 0.0
    return models_of(case, SimpleNamespace(M=M))


def models_of(case, o):
    """(model64, model_ld) from the tapped fields of a single fit's probe"""
    if case.wide and hasattr(o, "S"):
        m = wide_model(o.S, o.Sd, o.ct)
        return m, m
    m64 = narrow_model(o.M, case.scale, case.n, case.K, np.float64)
    if case.wide:                       # the host's stand-in for the scale kernel: float64 S is the operand itself
        return m64, m64
    return m64, narrow_model(o.M, case.scale, case.n, case.K, LD)


# The committed cases: (form, n, p, K, mix, options).  Every form runs the three mixes and a constant column with and without an l2
# term; the shapes are those at which the kernels change path (tests/test_gpu_covariance_path_passes.py says which is which).
def narrow_cases():
    out = [("cov", 60, p, 1, mix, {}) for p, mix in ((1, 1.0), (2, 0.5), (63, 1.0), (64, 0.0), (65, 0.5), (COV_MAX_FEATURES, 1.0))]
    out += [("cov", 60, 9, 1, 0.5, {}), ("cov", 60, 9, 1, 0.0, {}), ("cov", 40, 9, 1, 1.0, dict(constant=4)), ("cov", 40, 9, 1, 0.5, dict(constant=4)),
            ("cov", 120, 11, 1, 0.5, dict(sparse=True))]
    return out


def group_cases():
    shapes = [(1, 2), (9, 3), (16, 4), (13, 5), (86, 3), (5, 70), (mcov_max_features(2), 2), (mcov_max_features(10), 10)]
    mixes = [1.0, 0.5, 0.0, 0.5, 1.0, 0.5, 0.5, 1.0]
    out = [("mcov", 300 if p > 100 else 80, p, K, mix, {}) for (p, K), mix in zip(shapes, mixes)]
    out += [("mcov", 60, 9, 3, 1.0, {}), ("mcov", 60, 9, 3, 0.0, {}), ("mcov", 40, 9, 3, 1.0, dict(constant=4)), ("mcov", 40, 9, 3, 0.5, dict(constant=4))]
    return out


def wide_cases():
    ps = [1, 31, 33, 64, 65, 255, 256, 257, 1025, 1537, 1538]
    mixes = [1.0, 0.5, 0.0, 1.0, 0.5, 1.0, 0.0, 0.5, 1.0, 0.5, 1.0]
    out = [("wcov", 65, p, 1, mix, {}) for p, mix in zip(ps, mixes)]
    out += [("wcov", 40, 33, 1, 1.0, dict(constant=4)), ("wcov", 40, 33, 1, 0.5, dict(constant=4)), ("wcov", 50, 300, 1, RESCREEN_MIX["wcov"], dict(rescreen=True))]
    return out


def wide_group_cases():
    import wmcovariance_reference as wm
    mixes = [1.0, 0.5, 0.0, 1.0, 0.5, 0.0, 1.0, 0.5, 1.0]
    out = [("wmcov", n, p, K, mix, {}) for (n, p, K), mix in zip(wm.SHAPES, mixes)]
    out += [("wmcov", 40, 17, 3, 1.0, dict(constant=4)), ("wmcov", 40, 17, 3, 0.5, dict(constant=4)), ("wmcov", 50, 80, 2, RESCREEN_MIX["wmcov"], dict(rescreen=True))]
    return out


LIMIT_RATIOS = (0.6, 0.35)                # the feature limits: two lambdas, checks A, B and D


def limit_cases():
    return [("wcov", 40, WCOV_MAX_FEATURES, 1, 1.0, dict(limit=True)), ("wmcov", 40, wmcov_max_features(2), 2, 0.5, dict(limit=True))]


def build_case(spec):
    form, n, p, K, mix, opt = spec
    opt = dict(opt)
    if opt.pop("limit", False):
        opt["ratios"] = LIMIT_RATIOS
    if opt.pop("rescreen", False):
        import wcovariance_reference as wc
        import wmcovariance_reference as wm
        opt["xy"] = wc.rescreen_problem() if form == "wcov" else wm.rescreen_problem()
        opt["ratios"], opt["count_ratios"] = RESCREEN_REPLAY_RATIOS, RESCREEN_RATIOS[form]
    return make_case(form, n, p, K, mix, **opt)


# The re-screen inputs (wcovariance_reference.rescreen_problem, wmcovariance_reference.rescreen_problem): strongly correlated
# columns.  The replay's first-order bound doubles with every member of the list there (|S_kj| / S_jj is close to 1), so check
# D stays where the list is short.  Check E needs a lambda at which the list converges and the second screen still adds
# (test_covariance_path_reference.py asserts that it does: three screens) AND at most LONGEST sweeps at tol = 1e-7; at mix 0.5
# no path of four lambdas has both (the paths that re-screen take 300 to 1000 sweeps), so these two inputs run a small mix,
# where the l2 term shortens the sweeps and the l1 term still screens.
RESCREEN_MIX = {"wcov": 0.01, "wmcov": 0.05}
RESCREEN_REPLAY_RATIOS = (0.9, 0.75, 0.6, 0.7)
RESCREEN_RATIOS = {"wcov": (0.6, 0.2, 0.07, 0.2), "wmcov": (0.5, 0.1, 0.02, 0.05)}


def restated(case, model, **kw):
    """run(tol, max_iter, lam) of check_case through the float64 restatement on `model`"""
    kw.setdefault("order", "kernel" if case.listed else "sequential")
    return lambda tol, max_iter, lam: run_path(model, (1.0 - case.mix) * lam, case.mix * lam, case.ridge, tol, max_iter, blocks=case.blocks,
                                               listed=case.listed, **kw)


def case_id(spec):
    form, n, p, K, mix, opt = spec
    return f"{form}-n{n}-p{p}-K{K}-mix{mix}" + "".join(f"-{k}" for k in opt)


def all_cases():
    return narrow_cases() + group_cases() + wide_cases() + wide_group_cases()


# ---------------------------------------------------------------------------------------------------------------
# all checks of one single fit, given a function that runs the path kernel (the device, or a restatement)
# ---------------------------------------------------------------------------------------------------------------

def check_case(case, run, models, *, limit=False, report=None, order=None, cache=None, failures=None):
    """run(tol, max_iter, lam) -> fields W, G, sweeps, unconverged.  models: (model64, model_ld).  limit: A, B and D only.  cache: a
    dict that keeps the reference's own runs of check E between calls with the same models.  failures: a list that collects
    the message of every check that fails instead of stopping at the first (a violated precondition still stops)."""
    m64, mld = models
    kw = dict(blocks=case.blocks, listed=case.listed)

    def attempt(check, *a, **k):
        try:
            return check(*a, **k)
        except Precondition:
            raise
        except AssertionError as e:
            if failures is None:
                raise
            failures.append(str(e))

    one = run(REPLAY_TOL, 1, case.lam)
    attempt(check_outputs, one, mld, case.l2, case.l1, case.ridge, REPLAY_TOL, 1, blocks=case.blocks, what=f"{case.name} (one sweep)", optimum=False,
            report=report)
    attempt(check_replay, one, mld, case.l2, case.l1, case.ridge, REPLAY_TOL, what=case.name, report=report, **kw)
    if limit:
        return
    for setting in COUNT_SETTINGS:
        outs = attempt(check_counts, lambda tol, max_iter: run(tol, max_iter, case.lam_counts), m64, mld, case.l2_counts, case.l1_counts, case.ridge,
                       what=case.name, order=order, report=report, cache=cache, settings=[setting], **kw)
        tol, max_iter = setting
        o = outs[setting] if outs else run(tol, max_iter, case.lam_counts)
        attempt(check_outputs, o, mld, case.l2_counts, case.l1_counts, case.ridge, tol, max_iter, blocks=case.blocks,
                what=f"{case.name} (tol {tol}, max_iter {max_iter})", report=report)


# ---------------------------------------------------------------------------------------------------------------
# cross-validations: every job against its own training set and its own penalties
# ---------------------------------------------------------------------------------------------------------------

CV_MIXES = [0.5, 0.0]                    # one of them 0: ridge_jobs differs between the jobs
CV_GROUPS = 3
# (form, n, p, K): one shape per form from the single fits' lists, p odd; every training set keeps more rows than features
CV_FORMS = [("cov", 300, 65, 1), ("mcov", 120, 13, 5), ("wcov", 150, 33, 1), ("wmcov", 150, 17, 4)]


def cv_case(form, n, p, K, *, seed=0):
    """make_case's data with three groups of different sizes and the lambdas of the two mixes (A, L)"""
    case = make_case(form, n, p, K, 0.5, seed=seed)
    rng = np.random.default_rng(seed + 17)
    fold = rng.permutation(np.repeat([0, 1, 2], [2 * n // 5, n // 3, n - 2 * n // 5 - n // 3])).astype(np.int32)      # three sizes
    half = make_case(form, n, p, K, 0.5, seed=seed).lam
    zero = make_case(form, n, p, K, 0.0, seed=seed).lam
    case.fold, case.mixes, case.lams = fold, np.array(CV_MIXES), np.stack([half, zero])
    return case


def cv_response(case):
    """the response as a cross-validation takes it: (n,) for one response, (n, K) for mgaussian"""
    y = np.asarray(case.y, dtype=float).reshape(case.n, case.K)
    return y if case.multi else y[:, 0]


def cv_sets(case, train_on):
    return [np.flatnonzero((case.fold != t) if train_on == "rest" else (case.fold == t)) for t in range(CV_GROUPS)]


def cv_host_fields(case, train_on):
    """what the assembly stages hand the path kernel, formed on the host per training set: ([(model64, model_ld)], pen_a,
    pen_b, ridge) with the penalties in the units of each set's own response"""
    models, sds = [], []
    for rows in cv_sets(case, train_on):
        x, y = case.xd[rows], np.asarray(case.y, dtype=float).reshape(case.n, case.K)[rows]
        y = y - y.mean(axis=0)
        sd = y.std(axis=0)[0] if not case.multi else 1.0
        y = y / sd
        mean = x.mean(axis=0)
        var = ((x - mean) ** 2).mean(axis=0)
        sub = SimpleNamespace(xd=x, y=y, n=len(rows), K=case.K, scale=np.where(var == 0, 1.0, np.sqrt(var)), wide=case.wide)
        models.append(host_models(sub))
        sds.append(sd)
    sds = np.array(sds)
    pen_a = (1.0 - case.mixes)[:, None, None] * case.lams[:, None, :] / sds[None, :, None]
    pen_b = case.mixes[:, None, None] * case.lams[:, None, :] / sds[None, :, None]
    return models, pen_a, pen_b, np.repeat((case.mixes == 0.0)[:, None], CV_GROUPS, axis=1)


def cv_device_models(case, o):
    """[(model64, model_ld)] per training set from the tapped fields of sgdnet_cv_covariance_probe"""
    out = []
    for t in range(CV_GROUPS):
        if case.wide:
            m = wide_model(o.S[t], o.Sd[t], o.ct[t])
            out.append((m, m))
        else:
            out.append((narrow_model(o.Mt[t], o.scale[t], o.tstat[0, t], case.K, np.float64), narrow_model(o.Mt[t], o.scale[t], o.tstat[0, t], case.K, LD)))
    return out


def check_cv(case, run, fields_of, *, what, report=None):
    """run(tol, max_iter) -> the fields W, G, sweeps, unconverged with the leading axes (A, G); fields_of(o) -> (models, pen_a,
    pen_b, ridge) as the kernel got them.  Every job: A, B and D (against the long-double replay and, within twice its bound,
    against the float64 restatement handed the job's own inputs) at max_iter = 1; A, B, C and E at COUNT_SETTINGS."""
    kw = dict(blocks=case.blocks, listed=case.listed)
    one = run(REPLAY_TOL, 1)
    models, pen_a, pen_b, ridge = fields_of(one)
    A, G, L = pen_a.shape
    for a in range(A):
        for t in range(G):
            name = f"{what} job ({a}, {t})"
            job = job_of(one, a, t)
            check_outputs(job, models[t][1], pen_a[a, t], pen_b[a, t], bool(ridge[a, t]), REPLAY_TOL, 1, blocks=case.blocks, what=name, optimum=False,
                          report=report)
            check_replay(job, models[t][1], pen_a[a, t], pen_b[a, t], bool(ridge[a, t]), REPLAY_TOL, what=name, report=report, model64=models[t][0], **kw)
    for tol, max_iter in COUNT_SETTINGS:
        o = run(tol, max_iter)
        for a in range(A):
            for t in range(G):
                name = f"{what} job ({a}, {t})"
                job = job_of(o, a, t)
                check_counts(lambda *_: job, models[t][0], models[t][1], pen_a[a, t], pen_b[a, t], bool(ridge[a, t]), what=name, settings=[(tol, max_iter)],
                             report=report, **kw)
                check_outputs(job, models[t][1], pen_a[a, t], pen_b[a, t], bool(ridge[a, t]), tol, max_iter, blocks=case.blocks,
                              what=f"{name} (tol {tol}, max_iter {max_iter})", report=report)

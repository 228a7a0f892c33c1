"""Pure-numpy reference of the passes of one outer step of multinomial Newton mode (sgdnet_amd/csrc/mnewton.hip), shared
by tests/test_mnewton_reference.py (CPU) and tests/test_gpu_mnewton_passes.py (GPU): the long-double truth of every pass, a
rounding-error bound on |computed - truth| composed over the kernel's own arithmetic, float64 restatements of the kernels
(with the wrong formulas the bounds must reject), and the inputs both test modules use.

The error model, `Val`, the fl_* steps, gamma and fl_sum are those of tests/setup_reference.py; fl_exp, fl_log, the
summation orders, `inside` and the penalties are those of tests/newton_reference.py (imported, not copied): u = 2^-53, one
rounding per operation, a sum of m terms in ANY order errs by at most gamma_m sum|t_i|.  Every pass is checked in
isolation: its truth is formed from what the pass BEFORE it returned (the state pass from the returned mean and
a = u / scale; the moments from the returned mu and mean; the inner solve from the returned M), so a failure names one
kernel.  No tolerance in this file comes from what a device returned.

Coordinates: P = p + 1, Q = K P, coordinate (k, j) at k P + j, j = p the intercept of class k.  Class pair (k, l), k <= l, has
the index k K - k (k - 1) / 2 + (l - k): the upper triangle row by row.

State pass (mnewton_state_kernel, mnewton_finish_kernel), per sample i and class k:
    eta_k = sum_j fl(fl(x_ij - m_j) a_kj) + b_k     a sum of p + 1 terms: error E_k <= sum of the terms' own errors +
            gamma_(p+1) sum|terms| (fl_sum).
    mx    = max_k eta_k, computed exactly from the computed eta: |mx - max_k eta_k(true)| <= max_k E_k =: E_c.
    The softmax is shift invariant: mu_k = exp(eta_k - c) / sum_l exp(eta_l - c) for ANY c, and so is the loss,
    log sum_l exp(eta_l - c) + c - eta_y.  The truth is formed with c = the true maximum; the device's c is another
    number within E_c of it, so every quantity the device forms from its c is held to the truth's with E_c added where c
    enters: D_k = fl(eta_k - mx) errs by E_k + E_c + u |D_k|.  (E_c cancels in mu; the bound does not use that and is up
    to three times wider than it could be, which is still a rounding bound.)  Which class attains the maximum never matters.
    e_k   = exp(D_k)      1 ulp = 2 u relative (include/sgdnet_detmath.h) on top of e^D (e^E - 1); in the subnormal range
            the result is rescaled and rounded once more: two subnormal steps 2^-1073 absolute.  D < -745.2 gives 0.0
            exactly by that file's rule: where D + its bound < -746 the test asserts e = 0, hence mu = 0, bitwise.  The
            largest D is 0 to rounding: nothing overflows, whatever eta.
    s     = sum_k e_k     K terms in order, s >= 1 (the maximum's own term is exp(0));  mu_k = fl(e_k / s).
            The bounds on mu are absolute wherever a class underflows (a bound of 2^-1073 / s, not a relative one).  The
            true mu sum to 1, so each row's returned mu sum to 1 within the sum of the row's bounds.
    loss_i = fl(fl(log s + mx) - eta_y)     log: 1.5 ulp = 3 u relative (same file).
    mean loss: an any-order sum of n terms (threads stride, block_sum's tree, the workgroups in order), then / n.

Moments (mnewton_pair_tile_kernel, mnewton_pair_reduce_kernel).  For pair (k, l) and the RETURNED mu and mean the truth is
    M[a, b] = sum_i w_i d_ia d_ib,  M[a, p] = sum_i w_i d_ia,  d = [x - m | 1],  w = mu_k (1 - mu_k) if k = l else -mu_k mu_l,
    and for k = l:  M[a, p + 1] = sum_i (1{y_i = k} - mu_ik) d_ia.
    Per term the kernel rounds the deviations (fl_sub), 1 - mu_k (fl_sub), the weight product (fl_mul; the sign is exact),
    w d_b (fl_mul), the residual 1{y = k} - mu_k (fl_sub) and A B (fl_mul); the terms are then added 64 rows at a time in
    sequence (rows past the chunk's end are staged as exact zeros) and the chunks in order, an any-order sum of n terms:
    gamma_(n+2) times the sum of absolute terms (fl_sum; the 2 pays for the long-double reference).  The q column of an
    off-diagonal pair is staged as 0.0: the entry is 0.0 bitwise.

Inner solve (mnewton_cd_kernel).  The joint model is built in long double from the returned M:
    H[(k,a),(l,b)] = M[pair(min(k,l), max(k,l))][min(a,b), max(a,b)] / n / (s_a s_b),   q[(k,a)] = M[pair(k,k)][a, p+1] / n / s_a,
    s_p = 1, g(u) = H (u - u_cur) - q.  The kernel rounds three times per entry of H (two per entry of q).
  Optimality of the returned u (newton_reference.optimality over Q coordinates with K unpenalised intercepts), for every
  coordinate the kernel visited with a positive denominator:
    penalised, u_j = 0:  |g_j| <= l1 + B_j;    penalised, u_j != 0:  |g_j + l2 u_j + l1 sign u_j| <= B_j;    intercept:  |g_j| <= B_j.
    B_j = conv_j + drift_j + local_j (+ zero_j), as derived in newton_reference's docstring with Q updates a sweep:
      conv_j = sum_(c != j) |H_jc| tol max|u|,   drift_j = 2 u sweeps Q S_j,   local_j = 8 u (S_j + l1 + (|H_jj| + l2) max|u|),
      S_j = sum_c |H_jc| D + |q_j|,  D = 2 max(max|u - u_cur|, max|u|, max|u_cur|).
      zero_j  this kernel (not newton_cd_kernel) sets a thresholded coordinate with nu^2 H_jj <= kNewtonNegligible^2 to an
              exact zero.  Such a coordinate had |S(z)| = |nu| (H_jj + l2) <= kNewtonNegligible (H_jj + l2) / sqrt(H_jj) beyond
              its threshold: that much is added for penalised coordinates at 0 with H_jj > 0 when there is a threshold.
    A coordinate whose denominator is not positive stays at u_cur, bitwise (checked by the caller), and so does a frozen
    intercept.  Optimality is asserted only where the record says the solve converged; the callers assert the flag first
    wherever the case is known to converge.
  Single sweep (max_sweeps = 1): newton_reference.single_sweep_reference over Q coordinates, with the exact zero above:
    when the exact nu is within its own bound of that rule's threshold, the computed sweep may take either side, and
    |nu| is added to the coordinate's bound.
  Record: a = u / s is one IEEE division (bitwise); change and size are exact maxima; |w|^2 / 2 and |w|_1 run over the
    penalised coordinates only, at most 4 terms per lane in order (Q <= 199, 64 lanes) and a 6-step butterfly:
    gamma_(3+6+2) on top of the rounding of the squares."""
from types import SimpleNamespace

import numpy as np

from newton_reference import (CANDIDATES, LD_SLACK, NEGLIGIBLE, PENALTIES, SUMS, TINY, _all, _bro, _soft, blend_f64, fl_exp, fl_log,
                              inside, seq_sum)
from setup_reference import LD, U, Val, fl_add, fl_div, fl_mul, fl_sub, fl_sum, gamma

__all__ = ["CANDIDATES", "PENALTIES", "SUMS", "LD", "U", "Val", "NEGLIGIBLE", "LD_SLACK", "seq_sum", "inside"]

MAX_FEATURES = {2: 98, 3: 65, 4: 48, 5: 38, 10: 18, 99: 1}     # csrc/mnewton.hpp (the GPU test asserts the library agrees)
EXP_ZERO = -746.0                                              # below include/sgdnet_detmath.h's -745.2 with room to spare


def pair_index(k, l, K):
    return k * K - k * (k - 1) // 2 + (l - k)


def pair_list(K):
    return [(k, l) for k in range(K) for l in range(k, K)]


def _take(a, idx):
    return Val(a.v[idx], a.e[idx])


# ---------------------------------------------------------------------------------------------------------------
# state pass
# ---------------------------------------------------------------------------------------------------------------

def state_reference(xd, mean, a, y, K):
    """xd (n, p); mean (p,) and a (Q,): what the passes before returned.  eta, mu (Val, (n, K)), zero (bool (n, K): the
    device's e and mu are exactly 0.0 there), loss (Val)."""
    n, p = xd.shape
    P = p + 1
    A = np.asarray(a, dtype=LD).reshape(K, P)
    yi = np.asarray(y).astype(int)
    d = fl_sub(Val(xd.astype(LD)), Val(np.asarray(mean, dtype=LD)[None, :] + np.zeros((n, 1), dtype=LD)))
    term = fl_mul(Val(np.broadcast_to(d.v[:, None, :], (n, K, p)), np.broadcast_to(d.e[:, None, :], (n, K, p))),
                  Val(np.broadcast_to(A[None, :, :p], (n, K, p))))
    terms = Val(np.concatenate([term.v, np.broadcast_to(A[None, :, p:], (n, K, 1))], axis=2),
                np.concatenate([term.e, np.zeros((n, K, 1), dtype=LD)], axis=2))
    eta = fl_sum(terms, _all(terms.v.shape), 2)
    c = Val(np.broadcast_to(eta.v.max(axis=1)[:, None], (n, K)), np.broadcast_to(eta.e.max(axis=1)[:, None], (n, K)))
    D = fl_sub(eta, c)
    e = fl_exp(D)
    e = Val(e.v, e.e + TINY)
    zero = D.v + D.e < EXP_ZERO
    s = fl_sum(e, _all((n, K)), 1)
    mu = fl_div(e, _bro(Val(s.v[:, None], s.e[:, None]), (n, K)))
    rows = np.arange(n)
    li = fl_sub(fl_add(fl_log(s), Val(c.v[:, 0], c.e[:, 0])), Val(eta.v[rows, yi], eta.e[rows, yi]))
    loss = fl_div(fl_sum(li, _all(n), 0), Val(LD(n)))
    return SimpleNamespace(eta=eta, mu=mu, zero=zero, loss=loss)


def state_f64(xd, mean, a, y, K, fsum, wrong=None):
    """mnewton_state_kernel + mnewton_finish_kernel in float64; eta and s in the kernel's own order, the loss through fsum.
    wrong: "no_max" (the softmax without the row maximum), "loss_eta_0" (the loss takes eta of class 0)."""
    n, p = xd.shape
    A = np.asarray(a, dtype=np.float64).reshape(K, p + 1)
    yi = np.asarray(y).astype(int)
    eta = np.zeros((n, K))
    for j in range(p):
        eta = eta + (xd[:, j] - mean[j])[:, None] * A[None, :, j]
    eta = eta + A[None, :, p]
    mx = np.zeros(n) if wrong == "no_max" else eta.max(axis=1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(eta - mx[:, None])
        s = seq_sum(e.T)
        mu = e / s[:, None]
        li = (np.log(s) + mx) - eta[np.arange(n), 0 if wrong == "loss_eta_0" else yi]
    return SimpleNamespace(mu=mu, loss=float(fsum(li)) / n)


# ---------------------------------------------------------------------------------------------------------------
# moments
# ---------------------------------------------------------------------------------------------------------------

def moment_reference(xd, mean, mu, y, K):
    """Val of shape (pairs, p + 2, p + 2) from the returned mu (n, K) and mean; NaN where nothing is defined.  Defined:
    (a, b), a <= b <= p, for every pair; (a, p + 1), a <= p, for the diagonal pairs (the off-diagonal pairs' is exactly 0)."""
    n, p = xd.shape
    nc = p + 2
    pairs = pair_list(K)
    kk, ll = np.array([k for k, _ in pairs]), np.array([l for _, l in pairs])
    diag = kk == ll
    m = Val(np.asarray(mu, dtype=LD))
    one = Val(np.ones((n, len(pairs)), dtype=LD))
    mk, ml = _take(m, (slice(None), kk)), _take(m, (slice(None), ll))
    wd, wo = fl_mul(mk, fl_sub(one, mk)), fl_mul(mk, ml)
    w = Val(np.where(diag, wd.v, -wo.v), np.where(diag, wd.e, wo.e))                     # (n, pairs)
    ind = (np.asarray(y).astype(int)[:, None] == kk[None, :]).astype(LD)
    r = fl_sub(Val(ind), mk)
    r = Val(np.where(diag, r.v, 0), np.where(diag, r.e, 0))
    d = fl_sub(Val(xd.astype(LD)), Val(np.asarray(mean, dtype=LD)[None, :] + np.zeros((n, 1), dtype=LD)))
    A = Val(np.concatenate([d.v, np.ones((n, 1), dtype=LD)], axis=1), np.concatenate([d.e, np.zeros((n, 1), dtype=LD)], axis=1))
    shape = (n, len(pairs), p)
    wdev = fl_mul(_bro(Val(w.v[:, :, None], w.e[:, :, None]), shape), _bro(Val(d.v[:, None, :], d.e[:, None, :]), shape))
    B = Val(np.concatenate([wdev.v, w.v[:, :, None], r.v[:, :, None]], axis=2), np.concatenate([wdev.e, w.e[:, :, None], r.e[:, :, None]], axis=2))
    Tv, Te = np.full((len(pairs), nc, nc), LD(np.nan)), np.full((len(pairs), nc, nc), LD(np.nan))
    for a in range(p + 1):
        shp = (n, len(pairs), nc - a)
        s = fl_sum(fl_mul(_bro(Val(A.v[:, a, None, None], A.e[:, a, None, None]), shp), Val(B.v[:, :, a:], B.e[:, :, a:])), _all(shp), 0)
        Tv[:, a, a:], Te[:, a, a:] = s.v, s.e
    Tv[~diag, :, p + 1], Te[~diag, :, p + 1] = np.nan, np.nan
    return Val(Tv, Te)


def defined(K, p):
    """the entries of M a reference exists for"""
    k = np.zeros((len(pair_list(K)), p + 2, p + 2), dtype=bool)
    for a in range(p + 1):
        k[:, a, a:p + 1] = True
    for c, (i, j) in enumerate(pair_list(K)):
        k[c, :p + 1, p + 1] = i == j
    return k


def moments_f64(xd, mean, mu, y, K, fsum, wrong=None):
    """mnewton_pair_tile_kernel + mnewton_pair_reduce_kernel in float64.  wrong: "offdiag_plus" (the off-diagonal weight is
    +mu_k mu_l), "pairs_swapped" (K = 3: the blocks of (0, 2) and (1, 1) exchanged), "q_on_offdiag" (the q column staged on
    every pair), "q_uses_mu_l" (the residual of a diagonal pair (k, k) is taken with the mu of another class, the next one:
    what a kernel stages that reads mu_l after resolving the pair to the wrong l)."""
    n, p = xd.shape
    nc = p + 2
    d = xd - np.asarray(mean)[None, :]
    A = np.concatenate([d, np.ones((n, 1))], axis=1)
    yi = np.asarray(y).astype(int)
    M = np.full((len(pair_list(K)), nc, nc), np.nan)
    for c, (k, l) in enumerate(pair_list(K)):
        if k == l:
            w = mu[:, k] * (1.0 - mu[:, k])
        else:
            w = mu[:, k] * mu[:, l] if wrong == "offdiag_plus" else -(mu[:, k] * mu[:, l])
        r = np.zeros(n)
        if k == l or wrong == "q_on_offdiag":
            r = (yi == k).astype(np.float64) - mu[:, (k + 1) % K if wrong == "q_uses_mu_l" else k]
        B = np.concatenate([w[:, None] * d, w[:, None], r[:, None]], axis=1)
        for a in range(p + 1):
            M[c, a, a:] = fsum(A[:, a:a + 1] * B[:, a:])
    if wrong == "pairs_swapped":
        assert K == 3
        M[[2, 3]] = M[[3, 2]]
    return M


# ---------------------------------------------------------------------------------------------------------------
# inner solve
# ---------------------------------------------------------------------------------------------------------------

def joint_model(M, scale, n, K, dtype=LD, wrong=None):
    """H (Q x Q, symmetric) and q (Q) from the defined entries of the returned M, in `dtype`, in the kernel's order of
    operations.  wrong: "block_diagonal" (the off-diagonal class blocks are 0), "no_1_over_n" (H without / n; q keeps it),
    "scale_by_joint_index" (the scale of H taken at the joint index c, scale[c] for c < p and 1 beyond, not at c % P)."""
    F = dtype
    nc = M.shape[1]
    p, P = nc - 2, nc - 1
    Q = K * P
    kk, aa = np.divmod(np.arange(Q), P)
    s = np.concatenate([np.asarray(scale, dtype=F), [F(1)]])
    sa = s[aa]
    sH = np.where(np.arange(Q) < p, s[np.minimum(np.arange(Q), p)], F(1)) if wrong == "scale_by_joint_index" else sa
    k1, k2 = np.minimum(kk[:, None], kk[None, :]), np.maximum(kk[:, None], kk[None, :])
    a1, a2 = np.minimum(aa[:, None], aa[None, :]), np.maximum(aa[:, None], aa[None, :])
    Mf = np.asarray(M, dtype=F)
    H = Mf[k1 * K - k1 * (k1 - 1) // 2 + (k2 - k1), a1, a2]
    H = (H if wrong == "no_1_over_n" else H / F(n)) / (sH[:, None] * sH[None, :])
    if wrong == "block_diagonal":
        H = np.where(kk[:, None] == kk[None, :], H, F(0))
    q = Mf[kk * K - kk * (kk - 1) // 2, aa, p + 1] / F(n) / sa
    return H, q


def penalised(K, p):
    return np.arange(K * (p + 1)) % (p + 1) < p


def optimality(u, u_cur, H, q, pen, l2, l1, ridge, fit_intercept, tol, sweeps):
    """(residual, bound, visited, forced) as newton_reference.optimality, over Q coordinates of which pen are penalised;
    forced: thresholded coordinates without curvature but with an l2 term, which the kernel's exact-zero rule sets to 0.0
    whatever their gradient (H_jj = 0 makes nu^2 H_jj = 0): held to that, not to optimality."""
    Q = len(u)
    be = LD(0) if ridge else LD(l1)
    u, u_cur = np.asarray(u, dtype=LD), np.asarray(u_cur, dtype=LD)
    g = H @ (u - u_cur) - q
    res = np.where(pen & (u == 0), np.maximum(np.abs(g) - be, 0), np.abs(g + np.where(pen, LD(l2) * u + be * np.sign(u), 0)))
    umax = np.abs(u).max()
    D = 2 * max(np.abs(u - u_cur).max(), umax, np.abs(u_cur).max())
    aH = np.abs(H)
    S = aH.sum(axis=1) * D + np.abs(q)
    conv = (aH.sum(axis=1) - np.diag(aH)) * LD(tol) * umax
    drift = 2 * U * LD(sweeps) * Q * S
    den = np.diag(H) + np.where(pen, LD(l2), 0)
    local = 8 * U * (S + be + (np.diag(aH) + np.where(pen, LD(l2), 0)) * umax)
    hjj = np.diag(H)
    with np.errstate(divide="ignore", invalid="ignore"):
        zero = np.where(pen & (u == 0) & (hjj > 0) & (not ridge), LD(NEGLIGIBLE) * den / np.sqrt(np.where(hjj > 0, hjj, 1)), 0)
    visited = (den > 0) & (pen | bool(fit_intercept))
    forced = visited & pen & (hjj <= 0) & (not ridge)       # nu^2 H_jj = 0 <= the threshold: always the exact zero
    return res, conv + drift + local + zero, visited & ~forced, forced


def sweeps_f64(M, scale, n, K, u_cur, l2, l1, ridge, fit_intercept, max_sweeps, tol, wrong=None, dtype=np.float64):
    """mnewton_cd_kernel in float64 (wrong: those of joint_model).  Returns u, sweeps, converged, negligible."""
    F = dtype
    H, q = joint_model(M, scale, n, K, F, wrong)
    p = M.shape[1] - 2
    pen = penalised(K, p)
    Q = len(q)
    g = -q
    u = np.asarray(u_cur, dtype=F).copy()
    al, be = F(l2), F(0 if ridge else l1)
    lim = F(NEGLIGIBLE) * F(NEGLIGIBLE)
    sweeps, converged, negligible = 0, False, False
    while sweeps < max_sweeps and not converged:
        change = size = eta_sq = F(0)
        for j in range(Q):
            if not pen[j] and not fit_intercept:
                continue
            uj, hjj = u[j], H[j, j]
            z = hjj * uj - g[j]
            den = hjj + al if pen[j] else hjj
            nu = _soft(z, be) if (pen[j] and not ridge) else z
            nu = nu / den if den > 0 else uj
            with np.errstate(over="ignore"):
                if pen[j] and not ridge and den > 0 and nu * nu * hjj <= lim:
                    nu = F(0)
                d = nu - uj
                change, size, eta_sq = max(change, abs(d)), max(size, abs(nu)), max(eta_sq, nu * nu * hjj)
            if d != 0:
                u[j] = nu
                g = g + H[:, j] * d
        sweeps += 1
        negligible = bool(eta_sq <= lim)
        converged = bool((size == 0 and change == 0) or (size != 0 and change / size <= tol) or negligible)
    return u, sweeps, converged, negligible


def single_sweep_reference(M, scale, n, K, u_cur, l2, l1, ridge, fit_intercept):
    """One sweep in long double on the exact model of M, and the propagated bound E on a computed sweep's u (Val)."""
    H, q = joint_model(M, scale, n, K)
    p = M.shape[1] - 2
    pen = penalised(K, p)
    Q = len(q)
    EH = 3 * U * np.abs(H)
    g, Eg = -q.copy(), 2 * U * np.abs(q)
    u = np.asarray(u_cur, dtype=LD).copy()
    Eu = np.zeros(Q, dtype=LD)
    al, be = LD(l2), LD(0 if ridge else l1)
    for j in range(Q):
        if not pen[j] and not fit_intercept:
            continue
        uj, hjj = u[j], H[j, j]
        z = hjj * uj - g[j]
        den = hjj + al if pen[j] else hjj
        Ez = abs(uj) * EH[j, j] + Eg[j] + U * (abs(hjj * uj) + abs(z))
        sz = _soft(z, be) if (pen[j] and not ridge) else z
        if den > 0:
            Eden = EH[j, j] + U * den
            nu = sz / den
            Enu = (Ez + U * abs(sz) + abs(nu) * Eden) / (den - Eden) + U * abs(nu)
            if pen[j] and not ridge and hjj > 0 and (abs(nu) - Enu) * np.sqrt(hjj) <= LD(NEGLIGIBLE) * (1 + 8 * U):
                Enu = Enu + abs(nu)                      # the exact zero of the kernel: either side of its threshold
                if nu * nu * hjj <= LD(NEGLIGIBLE) ** 2:
                    nu = LD(0)
            elif pen[j] and not ridge and hjj <= 0:
                nu = LD(0)                               # nu * nu * 0 <= the threshold: always the exact zero
        else:
            nu, Enu = uj, LD(0)
        d = nu - uj
        Ed = Enu + U * abs(d)
        u[j], Eu[j] = nu, Enu
        upd = H[:, j] * d
        g = g + upd
        Eg = Eg + np.abs(H[:, j]) * Ed + abs(d) * EH[:, j] + U * np.abs(upd) + U * (np.abs(g) + Eg)
    return Val(u, LD(1.01) * Eu)


def record_reference(u, u_cur, scale, K):
    """what mnewton_publish leaves for the candidate u: a (exact), half_sq and abs (Val), change and size (exact)"""
    u, u_cur = np.asarray(u, dtype=np.float64), np.asarray(u_cur, dtype=np.float64)
    P = len(u) // K
    p = P - 1
    pen = penalised(K, p)
    w = Val(u[pen].astype(LD))
    depth = gamma(3 + 6 + 2)
    sq = fl_mul(w, w)
    half = Val(sq.v.sum() / 2, (sq.e.sum() + depth * (np.abs(sq.v) + sq.e).sum()) / 2)
    ab = Val(np.abs(w.v).sum(), depth * np.abs(w.v).sum())
    s = np.concatenate([np.asarray(scale, dtype=np.float64), [1.0]])
    a = np.where(pen, u / np.tile(s, K), u)
    return SimpleNamespace(a=a, half_sq=half, abs=ab, change=float(np.abs(u - u_cur).max()), size=float(np.abs(u).max()))


def record_f64(u, K, fsum, wrong=None):
    """mnewton_publish's two sums in float64 through fsum.  wrong = "penalty_with_intercepts": over all Q coordinates."""
    u = np.asarray(u, dtype=np.float64)
    w = u if wrong == "penalty_with_intercepts" else u[penalised(K, len(u) // K - 1)]
    with np.errstate(over="ignore"):                    # (a wrong formula's solve may diverge)
        return 0.5 * float(fsum(w * w)), float(fsum(np.abs(w)))


# ---------------------------------------------------------------------------------------------------------------
# inputs: the smallest that reach each edge (the GPU test and the CPU proof of the bounds use the same ones)
# ---------------------------------------------------------------------------------------------------------------

# p + 2 on both sides of a 16-column tile; n on both sides of the 64-row step, one, two and three chunks, several state
# workgroups at 1025
EDGE_SHAPES = [(1, 1, 2), (63, 13, 3), (64, 14, 2), (65, 15, 3), (257, 30, 4), (600, 6, 5), (1025, 33, 3)]
# p = None: the feature limit of K.  Q = 198 the largest reachable, Q = 199 prime, 4950 class pairs at K = 99
LIMIT_SHAPES = [(300, None, 2), (300, None, 3), (200, None, 10), (130, 1, 99)]
STRIDE_SHAPES = [(80, 20, 3), (80, 31, 2), (80, 12, 5)]            # Q = 63, 64, 65


def case(n, p, K, centre, empty_class=None, seed=0):
    """p = None: the feature limit.  Every class appears in y where n >= K, unless empty_class names one that has no member."""
    p = MAX_FEATURES[K] if p is None else p
    rng = np.random.default_rng(100000 * seed + 1000 * n + 10 * p + K)
    x = rng.standard_normal((n, p)) * rng.uniform(0.5, 3.0, p) + rng.uniform(-1.0, 1.0, p)
    y = rng.integers(0, K, n)
    if n >= K:
        y[rng.permutation(n)[:K]] = np.arange(K)
    if empty_class is not None:
        y[y == empty_class] = (empty_class + 1) % K
    u_cur = np.concatenate([0.1 * rng.standard_normal((K, p)) * (rng.random((K, p)) < 0.7), 0.2 * rng.standard_normal((K, 1))], axis=1).ravel()
    return SimpleNamespace(x=x, xd=x, centre=bool(centre), scale=rng.uniform(0.5, 2.0, p), y=y.astype(np.float64), K=K, u_cur=u_cur,
                           w0=rng.standard_normal((K, p)), n=n, p=p, P=p + 1, Q=K * (p + 1))


def candidate(c, kind):
    """(K, P) flat: zero coefficients with intercepts 0.3, 0, -0.3, ...; else w0 scaled so that the largest |eta| over
    samples and classes is CANDIDATES[kind] (about 3; about 40; 800: eta - max reaches below -745 and exp gives 0)."""
    target = CANDIDATES[kind]
    b = 0.3 * (1 - np.arange(c.K) % 3)
    if target == 0.0:
        return np.concatenate([np.zeros((c.K, c.p)), b[:, None]], axis=1).ravel()
    mean = c.xd.sum(axis=0) / c.n if c.centre else np.zeros(c.p)
    top = np.abs((c.xd - mean) @ (c.w0 / c.scale).T).max()
    w = c.w0 * (target / top) if top > 0 else c.w0
    return np.concatenate([w, (0.0 if kind == "overflow" else 1.0 / 3) * b[:, None]], axis=1).ravel()


def runs(shapes, kinds=tuple(CANDIDATES), centres=(0, 1)):
    """(n, p, K, centre, kind, penalty name): the penalties rotate with the candidates and the shapes"""
    names = [name for name, *_ in PENALTIES]
    return [(n, p, K, centre, kind, names[(i + j) % 3]) for i, (n, p, K) in enumerate(shapes) for centre in centres
            for j, kind in enumerate(kinds)]


def solve_plan(c, kind, pen):
    """how a case's inner solve is run and held: to convergence and optimality, or one sweep against the long-double sweep"""
    return dict(max_sweeps=1000, must_converge=True) if converges(c, kind, pen) else dict(max_sweeps=1)


def converges(c, kind, pen):
    """the cases whose inner solve must converge within kNewtonMaxSweeps at tol = 1e-7 (tests/test_mnewton_reference.py
    shows that the float64 restatement does): the zero and moderate candidates with any penalty, the wide one with an l2
    term at n > 1.  Elsewhere a single sweep is checked."""
    return kind in ("zero", "moderate") or (kind == "wide" and pen != "mix1" and c.n > 1)


# ---------------------------------------------------------------------------------------------------------------
# the checks: what sgdnet_amd.diagnostics.mnewton_probe returns (GPU), or restate() below (CPU), against the above
# ---------------------------------------------------------------------------------------------------------------

def check_candidate(u_out, a_out, rec, u_want, c, what):
    ref = record_reference(u_out, c.u_cur, c.scale, c.K)
    if u_want is not None:
        assert np.array_equal(u_out, u_want), f"{what}: u"
    assert np.array_equal(a_out, ref.a), f"{what}: a is not u / scale"
    assert rec["change"] == ref.change and rec["size"] == ref.size, f"{what}: change / size are not the exact maxima"
    inside(rec["half_sq"], ref.half_sq, f"{what}: half_sq")
    inside(rec["abs"], ref.abs, f"{what}: abs")


def check_publish(o, c, u, t):
    check_candidate(o.pub_u, o.pub_a, o.pub_rec, np.asarray(u, dtype=np.float64), c, "publish")
    want = blend_f64(c.u_cur, u, t)
    if t == 1.0 or np.frexp(t)[0] == 0.5:            # t (u - u_cur) is exact: the same bits with or without a fused multiply-add
        check_candidate(o.blend_u, o.blend_a, o.blend_rec, want, c, "blend")
    else:
        diff = np.abs(t * (np.asarray(u) - c.u_cur))
        inside(o.blend_u, Val(want.astype(LD), 3 * U * (np.abs(c.u_cur) + diff)), "blend: u")
        check_candidate(o.blend_u, o.blend_a, o.blend_rec, None, c, "blend")


def check_mean(o, c):
    if c.centre:
        inside(o.mean, fl_div(fl_sum(Val(c.xd.astype(LD)), _all(c.xd.shape), 0), Val(LD(c.n))), "mean")
    else:
        assert np.all(o.mean == 0.0), "mean: not exactly 0 without centring"


def check_state(o, c):
    """the state pass at a = o.pub_a with the means o.mean"""
    ref = state_reference(c.xd, o.mean, o.pub_a, c.y, c.K)
    assert np.all(np.isfinite(o.mu)) and np.isfinite(o.loss), "state: mu or the loss is not finite"
    inside(o.mu, ref.mu, "state: mu")
    assert np.all(o.mu[ref.zero] == 0.0), "state: mu is not exactly 0 where exp underflows"
    rowsum = np.asarray(o.mu, dtype=LD).sum(axis=1)
    assert np.all(np.abs(rowsum - 1) <= ref.mu.e.sum(axis=1)), "state: a row of mu does not sum to 1 within its bounds"
    inside(o.loss, ref.loss, "state: loss")
    return ref


def check_moments(o, c):
    """the moments pass from the returned mean and mu"""
    ref = moment_reference(c.xd, o.mean, o.mu, c.y, c.K)
    inside(o.M, ref, "moments: M", defined(c.K, c.p))
    for i, (k, l) in enumerate(pair_list(c.K)):
        if k != l:
            assert np.all(o.M[i, :c.p + 1, c.p + 1] == 0.0), f"moments: M: the q column of the off-diagonal pair ({k}, {l}) is not 0.0"
    return ref


def check_inner(o, c, l2, l1, ridge, fit_intercept, max_sweeps, tol, must_converge=False):
    """the inner solve on the returned M about u_cur"""
    p, K = c.p, c.K
    rec, u = o.cd_rec, o.cd_u
    check_candidate(o.cd_u, o.cd_a, rec, None, c, "inner")
    sweeps = int(rec["sweeps"])
    assert rec["sweeps"] == sweeps and 1 <= sweeps <= max_sweeps, f"inner: {rec['sweeps']} sweeps of at most {max_sweeps}"
    conv, negl = rec["converged"], rec["negligible"]
    assert conv in (0.0, 1.0) and negl in (0.0, 1.0) and (conv or not negl), f"inner: flags {conv}, {negl}"
    assert conv or sweeps == max_sweeps, "inner: stopped early without converging"
    if must_converge:
        assert conv == 1.0, f"inner: not converged after {sweeps} sweeps"
    H, q = joint_model(o.M, c.scale, c.n, K)
    pen = penalised(K, p)
    res, bound, visited, forced = optimality(u, c.u_cur, H, q, pen, l2, l1, ridge, fit_intercept, tol, sweeps)
    stays = ~visited & ~forced
    assert np.array_equal(u[stays], c.u_cur[stays]), "inner: a coordinate that is not visited, or has no curvature and no l2 term, moved"
    assert np.all(u[forced] == 0.0), "inner: a thresholded coordinate without curvature is not the exact zero"
    seen = pen | bool(fit_intercept)
    eta_sq = (np.asarray(u, dtype=LD) ** 2 * np.diag(H))[seen].max() if seen.any() else LD(0)
    lim = LD(NEGLIGIBLE) ** 2
    assert (eta_sq <= lim * (1 + 16 * U)) if negl else (eta_sq >= lim * (1 - 16 * U)), f"inner: negligible = {negl} at {float(eta_sq):.3e}"
    if conv and not negl and visited.any():
        k = int(np.argmax(np.where(visited, res - bound, -np.inf)))
        print(f"inner: {sweeps} sweeps, largest optimality residual {float(res[visited].max()):.3e}, bound at the worst {float(bound[k]):.3e}")
        assert np.all(res[visited] <= bound[visited]), f"inner: coordinate {k} misses optimality by {float(res[k]):.3e}, bound {float(bound[k]):.3e}"
    if max_sweeps == 1:
        one = single_sweep_reference(o.M, c.scale, c.n, K, c.u_cur, l2, l1, ridge, fit_intercept)
        inside(u, one, "inner: single sweep")
        f64 = sweeps_f64(o.M, c.scale, c.n, K, c.u_cur, l2, l1, ridge, fit_intercept, 1, tol)[0]
        inside(u, Val(f64.astype(LD), 2 * one.e), "inner: single sweep against float64 numpy")
        if fit_intercept:             # one sweep from u_cur: the sweep's own maxima are the record's
            ch, sz = rec["change"], rec["size"]
            want = (sz == 0 and ch == 0) or (sz != 0 and ch / sz <= tol) or bool(negl)
            assert bool(conv) == want, f"inner: converged = {conv} with change {ch}, size {sz}, negligible {negl}"


def check_probe(o, c, u, t, l2, l1, ridge, fit_intercept=True, max_sweeps=1000, tol=1e-7, must_converge=False):
    check_mean(o, c)
    check_publish(o, c, u, t)
    check_state(o, c)
    check_moments(o, c)
    check_inner(o, c, l2, l1, ridge, fit_intercept, max_sweeps, tol, must_converge)


def restate(c, u, t, l2, l1, ridge, fit_intercept=True, max_sweeps=1000, tol=1e-7, fsum=seq_sum, wrong=None):
    """One outer step in float64, every any-order sum through fsum: the fields of sgdnet_amd.diagnostics.mnewton_probe"""
    u = np.asarray(u, dtype=np.float64)
    K, p = c.K, c.p
    pen = penalised(K, p)
    s = np.tile(np.concatenate([c.scale, [1.0]]), K)
    o = SimpleNamespace(mean=np.array([fsum(c.xd[:, j]) / c.n if c.centre else 0.0 for j in range(p)]).reshape(p))

    def published(un):
        h, a = record_f64(un, K, fsum, wrong)
        return (un, np.where(pen, un / s, un), dict(half_sq=h, abs=a, change=float(np.abs(un - c.u_cur).max()), size=float(np.abs(un).max())))

    o.pub_u, o.pub_a, o.pub_rec = published(u.copy())
    o.blend_u, o.blend_a, o.blend_rec = published(blend_f64(c.u_cur, u, t))
    st = state_f64(c.xd, o.mean, o.pub_a, c.y, K, fsum, wrong)
    o.mu, o.loss = st.mu, st.loss
    o.M = moments_f64(c.xd, o.mean, o.mu, c.y, K, fsum, wrong)
    uc, sweeps, conv, negl = sweeps_f64(o.M, c.scale, c.n, K, c.u_cur, l2, l1, ridge, fit_intercept, max_sweeps, tol, wrong)
    o.cd_u, o.cd_a, rec = published(uc)
    o.cd_rec = dict(rec, loss=o.loss, sweeps=float(sweeps), converged=float(conv), negligible=float(negl))
    return o

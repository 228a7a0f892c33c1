"""Pure-numpy reference of the passes of one outer step of Newton mode (sgdnet_amd/csrc/newton.hip), shared by
tests/test_newton_reference.py (CPU) and tests/test_gpu_newton_passes.py (GPU): the long-double truth of every pass, a
rounding-error bound on |computed - truth| composed over the kernel's own arithmetic, float64 restatements of the
kernels (with the wrong formulas the bounds must reject), and the inputs both test modules use.

The error model, `Val`, the fl_* steps, gamma and fl_sum are those of tests/setup_reference.py (imported, not copied):
u = 2^-53, one rounding per operation, a sum of m terms in ANY order errs by at most gamma_m sum|t_i|.

Every pass is checked in isolation: its truth is formed from what the pass BEFORE it returned (the state pass from the
returned mean and a = u / scale; the moments from the returned v, r, mean, V and R; the inner solve from the returned
M), so a failure names one kernel.  No tolerance in this file comes from what a device returned.

State pass (newton_state_kernel, newton_finish_kernel), per sample:
    eta   = sum_j fl(fl(x_ij - m_j) a_j) + b   a sum of p + 1 terms.  The sparse centred walk adds ALL p terms, stored or
            not (an absent entry is the deviation -m_j); the sparse uncentred walk adds the stored ones only, the others
            being exact zeros: gamma_(p+1) over all p terms bounds every form.
    e     = exp(eta)      1 ulp = 2 u relative (include/sgdnet_detmath.h) on top of e^eta (e^E - 1) for the bound E on eta;
                          one subnormal step 2^-1074 absolute.  eta > 709.782712893384 gives +inf by that file's rule; an
                          input whose eta is within E of that threshold is refused (asserted), the rule being
                          discontinuous there.
    t     = 1 / (1 + e),  v = t (1 - t),  r = t - (1 - y)
            The bounds on v and r are ABSOLUTE, of the order of one unit roundoff of 1, not relative: for a very negative
            eta, t = 1 - e + ... rounds to within u of 1 and 1 - t is known to u only, however small e is.  That is what
            the composition through fl_sub gives; nothing relative can be promised for v << u.
            e = +inf: t = 0, v = 0, r = -(1 - y), all exact.
    loss  = log(1 + e) - y eta      log: 1.5 ulp = 3 u relative (same file); +inf where e is.
    mean loss, V = sum v, R = sum r: any-order sums of n terms (threads stride, block_sum's tree, the workgroups in order),
            the loss then divided by n.  V and R are taken against the long-double sums of the RETURNED v and r.

Moments.  Truth: sum_i v_i d_ij d_ik, sum_i v_i d_ij, sum_i r_i d_ij, sum v, sum r with d = x - m.
    dense   (newton_dense_tile_kernel + cov_reduce_kernel)  entry (a, b) = sum_i A_ia B_ib, A = [fl(x - m) | 1],
            B = [fl(v fl(x - m)) | v | r]: per term the roundings of the deviations and of two products, then an any-order
            sum of n terms (64-row steps in sequence, the chunks in order): gamma_(n+2) times the sum of absolute terms.
    sparse  (newton_sparse_pair_kernel)  the kernel does NOT add the centred terms.  It adds
                both = sum_{J and K} fl(fl(v d_j) d_k),  only_j = sum_{J \\ K} fl(v d_j),  only_k = sum_{K \\ J} fl(v d_k),
                v_union = sum_{J or K} v,    H_jk = ((both - m_k only_j) - m_j only_k) + ((V - v_union) m_j) m_k
            (V - v_union replaced by an exact 0 when j or k stores every row), and for the ones / q columns
                sum_J fl(w d_j) - m_j (W - sum_J w),   w = v or r, W = V or R   (0 for W - sum_J w when j is full).
            The truth is that identity in long double with the RETURNED V and R; the bound is composed over those terms,
            the cancellation in V - v_union included.  With a column of mean 1e6 that does not store every row the terms
            m_j m_k (V - v_union) and m_k only_j are 1e12 and 1e6 times the weights they multiply, and so are their
            roundings: a bound taken over the centred terms v d_j d_k of the stored rows alone would not cover them.

Inner solve (newton_cd_kernel).  The model is built in long double from the returned M:
    H_jk = M_jk / n / (s_j s_k),  q_j = M_(j,p+1) / n / s_j  (s_p = 1),  g(u) = H (u - u_cur) - q.
    The kernel rounds three times per entry of H (two per entry of q): 3 u |H_jk| (2 u |q_j|).
  Optimality of the returned u, for every coordinate the kernel visited with a positive denominator:
    penalised, u_j = 0:   |g_j| <= l1 + B_j;     penalised, u_j != 0:  |g_j + l2 u_j + l1 sign u_j| <= B_j;     intercept: |g_P| <= B_P.
    B_j = conv_j + drift_j + local_j:
      conv_j   A converged sweep (the flag, and not merely `negligible`) moved every coordinate by at most tol max|u|; when
               coordinate j was set, its condition held for the running gradient; the coordinates set after it moved g_j
               by at most sum_(k != j) |H_jk| tol max|u|.
      drift_j  The running g_j is updated P times a sweep, g_j += fl(H_jk d): two roundings each, at most
               u |H_jk d| + u |g_j| <= 2 u S_j with S_j = sum_k |H_jk| D + |q_j| as long as every intermediate iterate stays
               within D of u_cur.  D = 2 max(max|u - u_cur|, max|u|, max|u_cur|): coordinate descent never raises the
               convex model, so the iterates stay in the level set of the start; the factor 2 is the room given to that
               argument, stated here as the bound's assumption.  Over sweeps * P updates: 2 u sweeps P S_j.
      local_j  the update itself: z = fl(fl(H_jj u_j) - g_j), the threshold, the sum H_jj + l2, the division, and the
               rounding of H and q against the long-double model: 8 u (S_j + l1 + (|H_jj| + l2) max|u|).
  Single sweep (max_sweeps = 1): the sweep is carried out in long double with the exact H; the error of a computed sweep
    is propagated coordinate by coordinate (first order, times 1.01 for the second-order terms):
      E_z = |u_j| E_H + E_g_j + u (|H_jj u_j| + |z|),   E_nu = (E_z + u |S(z)| + |nu| E_den) / (den - E_den) + u |nu|,
      E_d = E_nu + u |d|,   E_g_k += |H_kj| E_d + |d| E_H_kj + u |H_kj d| + u (|g_k| + E_g_k)
    (the soft threshold S is 1-Lipschitz; E_H = 3 u |H|; E_g starts at 2 u |q|).  The device is held to E against the
    long-double sweep, a float64 numpy sweep as well, so the two are within 2 E of each other.
  Record: a_k = u_k / s_k is one IEEE division (bitwise); change and size are exact maxima; |w|^2 / 2 and |w|_1 are sums of
    at most 4 terms per lane in order and a 6-step butterfly: gamma_(3+6+2) on top of the rounding of the squares."""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

from setup_reference import LD, U, Val, fl_add, fl_div, fl_mul, fl_sub, fl_sum, gamma

EXP_OVERFLOW = 709.782712893384          # include/sgdnet_detmath.h: above it exp() is +inf
NEGLIGIBLE = 16 * 2.220446049250313e-16  # csrc/newton.hpp: kNewtonNegligible
TINY = LD(2.0) ** -1074
LD_SLACK = LD(2.0) ** -60                # numpy's long-double exp / log: a few units in their own last place


def _bro(a, shape):
    return Val(np.broadcast_to(a.v, shape), np.broadcast_to(a.e, shape))


def _all(shape):
    return np.ones(shape, dtype=bool)


def fl_exp(a):
    v = np.exp(a.v)
    e = v * np.expm1(a.e)
    return Val(v, e + (2 * U + LD_SLACK) * (v + e) + TINY)


def fl_log(a):
    assert np.all(a.v - a.e > 0)
    v = np.log(a.v)
    e = a.e / (a.v - a.e)
    return Val(v, e + (3 * U + LD_SLACK) * (np.abs(v) + e))


# ---------------------------------------------------------------------------------------------------------------
# summation orders of the float64 restatements (along axis 0)
# ---------------------------------------------------------------------------------------------------------------

def seq_sum(t):
    t = np.asarray(t, dtype=np.float64)
    return np.add.accumulate(t, axis=0)[-1] if len(t) else np.zeros(t.shape[1:])


def pair_sum(t):
    t = np.asarray(t, dtype=np.float64)
    if len(t) <= 2:
        return seq_sum(t)
    h = len(t) // 2
    return pair_sum(t[:h]) + pair_sum(t[h:])


def block_sum(t):
    """the kernels' shape: thread i adds t[i], t[i + 256], ... in order; then block_sum's tree sh[i] += sh[i + s]"""
    t = np.asarray(t, dtype=np.float64)
    pad = (-len(t)) % 256 if len(t) else 256
    t = np.concatenate([t, np.zeros((pad,) + t.shape[1:])])
    sh = seq_sum(t.reshape((-1, 256) + t.shape[1:]))
    s = 128
    while s > 0:
        sh = sh[:s] + sh[s:2 * s]
        s >>= 1
    return sh[0]


SUMS = {"sequential": seq_sum, "pairwise": pair_sum, "strided256": block_sum}


# ---------------------------------------------------------------------------------------------------------------
# means
# ---------------------------------------------------------------------------------------------------------------

def mean_reference(xd, stored, centre):
    """cov_sum_kernel: sum of the stored values (dense: all) in any order, divided by n; exactly 0 without centring"""
    n, p = xd.shape
    if not centre:
        return Val(np.zeros(p, dtype=LD))
    return fl_div(fl_sum(Val(xd.astype(LD)), stored, 0), Val(LD(n)))


def mean_f64(xd, stored, centre, fsum):
    n, p = xd.shape
    return np.array([fsum(xd[stored[:, j], j]) / n if centre else 0.0 for j in range(p)]).reshape(p)


# ---------------------------------------------------------------------------------------------------------------
# state pass
# ---------------------------------------------------------------------------------------------------------------

def state_reference(xd, mean, a, y):
    """xd: (n, p) float64, the dense form of x; mean (p,) and a (p + 1,): what the passes before returned.
    Returns eta, v, r (Val, per sample), overflow (bool per sample), loss (Val of the mean loss; v = inf with overflow)."""
    n, p = xd.shape
    y = np.asarray(y, dtype=LD)
    d = fl_sub(Val(xd.astype(LD)), Val(np.asarray(mean, dtype=LD)[None, :] + np.zeros((n, 1), dtype=LD)))
    term = fl_mul(d, Val(np.asarray(a[:p], dtype=LD)[None, :] + np.zeros((n, 1), dtype=LD)))
    terms = Val(np.concatenate([term.v, np.full((n, 1), LD(a[p]))], axis=1), np.concatenate([term.e, np.zeros((n, 1), dtype=LD)], axis=1))
    eta = fl_sum(terms, _all(terms.v.shape), 1)
    assert np.all(np.abs(eta.v - EXP_OVERFLOW) > eta.e), "an eta too close to the overflow threshold of exp()"
    over = eta.v > EXP_OVERFLOW
    safe = Val(np.where(over, 0, eta.v), np.where(over, 0, eta.e))
    one = Val(np.ones(n, dtype=LD))
    s = fl_add(one, fl_exp(safe))
    t = fl_div(one, s)
    v = fl_mul(t, fl_sub(one, t))
    r = fl_sub(t, Val(1 - y))                          # 1 - y is exact for class codes
    li = fl_sub(fl_log(s), fl_mul(Val(y), safe))
    v = Val(np.where(over, 0, v.v), np.where(over, 0, v.e))
    r = Val(np.where(over, y - 1, r.v), np.where(over, 0, r.e))
    if over.any():
        loss = Val(LD(np.inf))
    else:
        loss = fl_div(fl_sum(li, _all(n), 0), Val(LD(n)))
    return SimpleNamespace(eta=eta, v=v, r=r, overflow=over, loss=loss)


def sum_reference(w):
    """V or R: the long-double sum of the returned weights and the any-order bound over n terms"""
    w = Val(np.asarray(w, dtype=LD))
    return fl_sum(w, _all(w.v.shape), 0)


def state_f64(xd, stored, centre, mean, a, y, fsum, wrong=None):
    """newton_state_kernel + newton_finish_kernel in float64; the sums of loss, v and r through fsum, eta in the kernel's
    own order.  wrong = "v_is_t_squared": v = t * t."""
    n, p = xd.shape
    eta = np.zeros(n)
    for j in range(p):
        d = xd[:, j] - mean[j]
        if centre:
            d = np.where(stored[:, j], d, -mean[j])
        eta = eta + d * a[j]
    eta = eta + a[p]
    with np.errstate(over="ignore"):
        e = np.where(eta > EXP_OVERFLOW, np.inf, np.exp(eta))
        t = 1.0 / (1.0 + e)
        v = t * t if wrong == "v_is_t_squared" else t * (1.0 - t)
        r = t - (1.0 - y)
        li = np.log(1.0 + e) - y * eta
    return SimpleNamespace(v=v, r=r, loss=float(fsum(li)) / n, V=float(fsum(v)), R=float(fsum(r)))


# ---------------------------------------------------------------------------------------------------------------
# moments
# ---------------------------------------------------------------------------------------------------------------

def dense_moment_reference(xd, mean, v, r):
    """Val of shape (p + 2, p + 2); rows 0 .. p, columns >= the row are defined (the rest is NaN)"""
    n, p = xd.shape
    nc = p + 2
    d = fl_sub(Val(xd.astype(LD)), Val(np.asarray(mean, dtype=LD)[None, :] + np.zeros((n, 1), dtype=LD)))
    vv = Val(np.asarray(v, dtype=LD)[:, None] + np.zeros((1, p), dtype=LD))
    vd = fl_mul(vv, d)
    A = Val(np.concatenate([d.v, np.ones((n, 1), dtype=LD)], axis=1), np.concatenate([d.e, np.zeros((n, 1), dtype=LD)], axis=1))
    B = Val(np.concatenate([vd.v, np.asarray(v, dtype=LD)[:, None], np.asarray(r, dtype=LD)[:, None]], axis=1),
            np.concatenate([vd.e, np.zeros((n, 2), dtype=LD)], axis=1))
    Tv, Te = np.full((nc, nc), LD(np.nan)), np.full((nc, nc), LD(np.nan))
    for a in range(p + 1):
        Aa = _bro(Val(A.v[:, a:a + 1], A.e[:, a:a + 1]), (n, nc - a))
        s = fl_sum(fl_mul(Aa, Val(B.v[:, a:], B.e[:, a:])), _all((n, nc - a)), 0)
        Tv[a, a:], Te[a, a:] = s.v, s.e
    return Val(Tv, Te)


def dense_moments_f64(xd, mean, v, r, fsum, wrong=None):
    """newton_dense_tile_kernel + cov_reduce_kernel in float64.  wrong = "q_staged_as_vr": tile column p + 1 is v * r."""
    n, p = xd.shape
    nc = p + 2
    d = xd - mean[None, :]
    qcol = v * r if wrong == "q_staged_as_vr" else r
    A = np.concatenate([d, np.ones((n, 1))], axis=1)
    B = np.concatenate([v[:, None] * d, v[:, None], qcol[:, None]], axis=1)
    M = np.full((nc, nc), np.nan)
    for a in range(p + 1):
        M[a, a:] = fsum(A[:, a:a + 1] * B[:, a:])
    return M


def sparse_moment_reference(xd, stored, mean, v, r, V, R):
    """The kernel's identity in long double with the returned V and R, and the bound over the terms it adds."""
    n, p = xd.shape
    nc = p + 2
    m = np.asarray(mean, dtype=LD)
    d = fl_sub(Val(xd.astype(LD)), Val(m[None, :] + np.zeros((n, 1), dtype=LD)))
    full_col = stored.sum(axis=0) == n
    Tv, Te = np.full((nc, nc), LD(np.nan)), np.full((nc, nc), LD(np.nan))
    for j in range(p):
        w = p - j
        J = np.broadcast_to(stored[:, j:j + 1], (n, w))
        K = stored[:, j:]
        dj = _bro(Val(d.v[:, j:j + 1], d.e[:, j:j + 1]), (n, w))
        dk = Val(d.v[:, j:], d.e[:, j:])
        vv = Val(np.asarray(v, dtype=LD)[:, None] + np.zeros((1, w), dtype=LD))
        vdj = fl_mul(vv, dj)
        both = fl_sum(fl_mul(vdj, dk), J & K, 0)
        only_j = fl_sum(vdj, J & ~K, 0)
        only_k = fl_sum(fl_mul(vv, dk), K & ~J, 0)
        v_union = fl_sum(vv, J | K, 0)
        full = full_col[j] | full_col[j:]
        nei = fl_sub(Val(np.full(w, LD(V))), v_union)
        nei = Val(np.where(full, 0, nei.v), np.where(full, 0, nei.e))
        mj, mk = Val(np.full(w, m[j])), Val(m[j:])
        h = fl_add(fl_sub(fl_sub(both, fl_mul(mk, only_j)), fl_mul(mj, only_k)), fl_mul(fl_mul(nei, mj), mk))
        Tv[j, j:p], Te[j, j:p] = h.v, h.e
        for c, (wt, total) in enumerate(((v, V), (r, R))):
            ww = Val(np.asarray(wt, dtype=LD))
            dj1 = Val(d.v[:, j], d.e[:, j])
            a = fl_sum(fl_mul(ww, dj1), stored[:, j], 0)
            ws = fl_sum(ww, stored[:, j], 0)
            rest = Val(LD(0)) if full_col[j] else fl_sub(Val(LD(total)), ws)
            e = fl_sub(a, fl_mul(Val(m[j]), rest))
            Tv[j, p + c], Te[j, p + c] = e.v, e.e
    Tv[p, p], Te[p, p], Tv[p, p + 1], Te[p, p + 1] = LD(V), 0, LD(R), 0      # copied, bit for bit
    return Val(Tv, Te)


def centred_moment_truth(xd, mean, v, r):
    """sum_i w_i d_ij d_ik over ALL rows, in long double: what the sparse identity equals when V and R are the exact sums"""
    n, p = xd.shape
    D = np.concatenate([xd.astype(LD) - np.asarray(mean, dtype=LD)[None, :], np.ones((n, 1), dtype=LD)], axis=1)
    T = np.full((p + 2, p + 2), LD(np.nan))
    T[:p + 1, :p + 1] = (D * np.asarray(v, dtype=LD)[:, None]).T @ D
    T[:p + 1, p + 1] = D.T @ np.asarray(r, dtype=LD)
    return T


def sparse_moments_f64(xd, stored, mean, v, r, V, R, fsum, wrong=None):
    """newton_sparse_pair_kernel in float64.  wrong: "neither_dropped" (no (V - v_union) m_j m_k term),
    "only_k_unweighted" (only_k summed with weight 1), "full_shortcut_always" (the ones / q columns take the shortcut of a
    full column whether it is full or not), "V_for_R" (q_j uses V where R belongs)."""
    n, p = xd.shape
    nc = p + 2
    M = np.full((nc, nc), np.nan)
    full_col = stored.sum(axis=0) == n
    for j in range(p):
        J = stored[:, j]
        dj = xd[:, j] - mean[j]
        for k in range(j, p):
            K = stored[:, k]
            dk = xd[:, k] - mean[k]
            both = fsum((v * dj * dk)[J & K])
            only_j = fsum((v * dj)[J & ~K])
            only_k = fsum(((1.0 if wrong == "only_k_unweighted" else v) * dk)[K & ~J])
            v_union = fsum(v[J | K])
            nei = 0.0 if (full_col[j] or full_col[k] or wrong == "neither_dropped") else V - v_union
            M[j, k] = both - mean[k] * only_j - mean[j] * only_k + nei * mean[j] * mean[k]
        for c, (wt, total) in enumerate(((v, V), (r, V if wrong == "V_for_R" else R))):
            a, ws = fsum((wt * dj)[J]), fsum(wt[J])
            M[j, p + c] = a - mean[j] * (0.0 if (full_col[j] or wrong == "full_shortcut_always") else total - ws)
    M[p, p], M[p, p + 1] = V, R
    return M


def upper(nc):
    """the defined entries of M: rows 0 .. p - 1 from the diagonal on, and the corners (p, p), (p, p + 1)"""
    k = np.zeros((nc, nc), dtype=bool)
    for j in range(nc - 1):
        k[j, j:] = True
    return k


# ---------------------------------------------------------------------------------------------------------------
# inner solve
# ---------------------------------------------------------------------------------------------------------------

def model_from_M(M, scale, n):
    """H (P x P, symmetric) and q (P) in long double from the upper triangle of the returned M"""
    nc = M.shape[0]
    p, P = nc - 2, nc - 1
    s = np.concatenate([np.asarray(scale, dtype=LD), [LD(1)]])
    Mu = np.asarray(M, dtype=LD)[:P, :P]
    Mu = np.triu(Mu) + np.triu(Mu, 1).T
    return Mu / LD(n) / np.outer(s, s), np.asarray(M, dtype=LD)[:P, p + 1] / LD(n) / s


def optimality(u, u_cur, H, q, l2, l1, ridge, fit_intercept, tol, sweeps):
    """(residual, bound, visited): residual_j is the amount by which coordinate j misses its optimality condition for
    the model (H, q) about u_cur; bound_j = conv + drift + local of the module docstring; visited: the coordinates the
    kernel sets with a positive denominator (the others stay, or go to 0: checked by the caller)."""
    P = len(u)
    p = P - 1
    be = LD(0) if ridge else LD(l1)
    u, u_cur = np.asarray(u, dtype=LD), np.asarray(u_cur, dtype=LD)
    g = H @ (u - u_cur) - q
    pen = np.arange(P) < p
    res = np.where(pen & (u == 0), np.maximum(np.abs(g) - be, 0), np.abs(g + np.where(pen, LD(l2) * u + be * np.sign(u), 0)))
    umax = np.abs(u).max()
    D = 2 * max(np.abs(u - u_cur).max(), umax, np.abs(u_cur).max())
    aH = np.abs(H)
    S = aH.sum(axis=1) * D + np.abs(q)
    conv = (aH.sum(axis=1) - np.diag(aH)) * LD(tol) * umax
    drift = 2 * U * LD(sweeps) * P * S
    local = 8 * U * (S + be + (np.diag(aH) + np.where(pen, LD(l2), 0)) * umax)
    den = np.diag(H) + np.where(pen, LD(l2), 0)
    visited = (den > 0) & (pen | bool(fit_intercept))
    return res, conv + drift + local, visited


def _soft(z, be):
    return z - be if z > be else (z + be if z < -be else z * 0)


def sweeps_f64(M, scale, n, u_cur, l2, l1, ridge, fit_intercept, max_sweeps, tol, wrong=None, dtype=np.float64):
    """newton_cd_kernel in float64 (dtype = np.longdouble: the same sweeps in long double).  wrong = "no_1_over_n": H
    loaded without the division by n.  Returns u, sweeps, converged, negligible."""
    F = dtype
    nc = M.shape[0]
    p, P = nc - 2, nc - 1
    s = np.concatenate([np.asarray(scale, dtype=F), [F(1)]])
    Mu = np.asarray(M, dtype=F)[:P, :P]
    Mu = np.triu(Mu) + np.triu(Mu, 1).T
    dn = F(n)
    H = (Mu if wrong == "no_1_over_n" else Mu / dn) / np.outer(s, s)
    g = -(np.asarray(M, dtype=F)[:P, p + 1] / dn / s)
    u = np.asarray(u_cur, dtype=F).copy()
    al, be = F(l2), F(0 if ridge else l1)
    n_coord = P if fit_intercept else p
    sweeps, converged, negligible = 0, False, False
    while sweeps < max_sweeps and not converged:
        change = size = eta_sq = F(0)
        for j in range(n_coord):                      # (an overflowing nu * nu * hjj is +inf here as on the device)
            pen = j < p
            uj, hjj = u[j], H[j, j]
            z = hjj * uj - g[j]
            den = hjj + al if pen else hjj
            nu = _soft(z, be) if (pen and not ridge) else z
            nu = nu / den if den > 0 else (F(0) if pen else uj)
            d = nu - uj
            with np.errstate(over="ignore"):
                change, size, eta_sq = max(change, abs(d)), max(size, abs(nu)), max(eta_sq, nu * nu * hjj)
            if d != 0:
                u[j] = nu
                g = g + H[:, j] * d
        sweeps += 1
        negligible = bool(eta_sq <= F(NEGLIGIBLE) * F(NEGLIGIBLE))
        converged = bool((size == 0 and change == 0) or (size != 0 and change / size <= tol) or negligible)
    return u, sweeps, converged, negligible


def single_sweep_reference(M, scale, n, u_cur, l2, l1, ridge, fit_intercept):
    """One sweep in long double on the exact model of M, and the propagated bound E on a computed sweep's u (Val)."""
    H, q = model_from_M(M, scale, n)
    P = len(q)
    p = P - 1
    EH = 3 * U * np.abs(H)
    g, Eg = -q.copy(), 2 * U * np.abs(q)
    u = np.asarray(u_cur, dtype=LD).copy()
    Eu = np.zeros(P, dtype=LD)
    al, be = LD(l2), LD(0 if ridge else l1)
    for j in range(P if fit_intercept else p):
        pen = j < p
        uj, hjj = u[j], H[j, j]
        z = hjj * uj - g[j]
        den = hjj + al if pen else hjj
        Ez = abs(uj) * EH[j, j] + Eg[j] + U * (abs(hjj * uj) + abs(z))
        sz = _soft(z, be) if (pen and not ridge) else z
        if den > 0:
            Eden = EH[j, j] + U * den
            nu = sz / den
            Enu = (Ez + U * abs(sz) + abs(nu) * Eden) / (den - Eden) + U * abs(nu)
        else:
            nu, Enu = (LD(0) if pen else uj), LD(0)
        d = nu - uj
        Ed = Enu + U * abs(d)
        u[j], Eu[j] = nu, Enu
        upd = H[:, j] * d
        g = g + upd
        Eg = Eg + np.abs(H[:, j]) * Ed + abs(d) * EH[:, j] + U * np.abs(upd) + U * (np.abs(g) + Eg)
    return Val(u, LD(1.01) * Eu)


def record_reference(u, u_cur, scale):
    """what publish_candidate leaves for the candidate u: a (exact), half_sq and abs (Val), change and size (exact)"""
    u, u_cur = np.asarray(u, dtype=np.float64), np.asarray(u_cur, dtype=np.float64)
    p = len(u) - 1
    w = Val(u[:p].astype(LD))
    depth = gamma(3 + 6 + 2)
    sq = fl_mul(w, w)
    half = Val(sq.v.sum() / 2, (sq.e.sum() + depth * (np.abs(sq.v) + sq.e).sum()) / 2)
    ab = Val(np.abs(w.v).sum(), depth * np.abs(w.v).sum())
    a = np.concatenate([u[:p] / np.asarray(scale, dtype=np.float64), u[p:]])
    return SimpleNamespace(a=a, half_sq=half, abs=ab, change=float(np.abs(u - u_cur).max()), size=float(np.abs(u).max()))


def record_f64(u, fsum):
    """publish_candidate's two sums in float64 through fsum"""
    w = np.asarray(u, dtype=np.float64)[:-1]
    return 0.5 * float(fsum(w * w)), float(fsum(np.abs(w)))


def blend_f64(u_cur, u, t):
    """newton_blend_kernel: u itself at t = 1, else u_cur + t (u - u_cur), three IEEE operations"""
    u_cur, u = np.asarray(u_cur, dtype=np.float64), np.asarray(u, dtype=np.float64)
    return u.copy() if t == 1.0 else u_cur + t * (u - u_cur)


# ---------------------------------------------------------------------------------------------------------------
# inputs: the smallest that reach each edge (the GPU test and the CPU proof of the bounds use the same ones)
# ---------------------------------------------------------------------------------------------------------------

DENSE_SHAPES = [(1, 1), (63, 14), (64, 15), (65, 16), (257, 30), (1025, 33), (300, None)]   # None: sgdnet_newton_max_features()
MAX_FEATURES = 198                       # csrc/newton.hpp: kNewtonMaxFeatures (the GPU test asserts the library agrees)
SPARSE_N = [1, 255, 256, 257, 600]
CANDIDATES = {"zero": 0.0, "moderate": 3.0, "wide": 40.0, "overflow": 800.0}   # the largest |eta| the candidate gives
SPARSE_COLUMNS = ("empty", "full", "one_entry", "long", "same_a", "same_b", "disjoint_a", "disjoint_b", "explicit_zeros",
                  "mean_1e6_full", "mean_1e6_part")


def dense_case(n, p, centre):
    """p = None: the feature limit.  p + 1 and p + 2 on both sides of a 16-column tile; n on both sides of the 64-row
    staging step and of the one-chunk / two-chunk boundary of dense_rows_per_chunk (256 rows)."""
    p = MAX_FEATURES if p is None else p
    rng = np.random.default_rng(1000 * n + p)
    x = rng.standard_normal((n, p)) * rng.uniform(0.5, 3.0, p) + rng.uniform(-1.0, 1.0, p)
    return _finish_case(rng, x, x, np.ones((n, p), dtype=bool), centre, rng.uniform(0.5, 2.0, p))


def sparse_case(n, centre, descending=False):
    """n x 11 (SPARSE_COLUMNS): an empty column, a full one, one entry, more than 256 entries where n allows, two columns
    with identical supports, two with disjoint supports, stored explicit zeros, and two columns of mean 1e6 with unit
    spread, one full and one storing 9 rows in 10.  descending: the row indices of every column in descending order."""
    rng = np.random.default_rng(7000 + n)

    def rows(k):
        return np.sort(rng.choice(n, min(max(k, 1), n), replace=False))

    def vals(k):
        return rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)

    perm = rng.permutation(n)
    same = rows(n // 3)
    zr = rows(n // 2)
    zv = vals(len(zr)) * (np.arange(len(zr)) % 2)
    part = rows(9 * n // 10)
    cols = {"empty": (np.zeros(0, dtype=int), np.zeros(0)), "full": (np.arange(n), vals(n)),
            "one_entry": (rows(1), vals(1)), "long": (rows(300 if n > 256 else n // 2), None),
            "same_a": (same, vals(len(same))), "same_b": (same, vals(len(same))),
            "disjoint_a": (np.sort(perm[:(n + 1) // 2]), None), "disjoint_b": (np.sort(perm[(n + 1) // 2:]), None),
            "explicit_zeros": (zr, zv), "mean_1e6_full": (np.arange(n), 1e6 + rng.standard_normal(n)),
            "mean_1e6_part": (part, 1e6 + rng.standard_normal(len(part)))}
    indptr, indices, data = [0], [], []
    for name in SPARSE_COLUMNS:
        r, v = cols[name]
        v = vals(len(r)) if v is None else v
        if descending:
            r, v = r[::-1], v[::-1]
        indices.append(r)
        data.append(v)
        indptr.append(indptr[-1] + len(r))
    x = sp.csc_matrix((np.concatenate(data), np.concatenate(indices).astype(np.int32), np.array(indptr, dtype=np.int32)),
                      shape=(n, len(SPARSE_COLUMNS)))
    scale = rng.uniform(0.5, 2.0, x.shape[1])
    scale[-2:] = 1.0
    return _finish_case(rng, x, *_dense_and_stored(x), centre, scale)


def empty_sparse_case(n, p, centre):
    """nnz = 0"""
    rng = np.random.default_rng(9000 + n)
    x = sp.csc_matrix((n, p))
    return _finish_case(rng, x, *_dense_and_stored(x), centre, rng.uniform(0.5, 2.0, p))


def _dense_and_stored(x):
    n, p = x.shape
    xd, stored = np.zeros((n, p)), np.zeros((n, p), dtype=bool)
    for j in range(p):
        q = slice(x.indptr[j], x.indptr[j + 1])
        xd[x.indices[q], j] = x.data[q]
        stored[x.indices[q], j] = True
    return xd, stored


def _finish_case(rng, x, xd, stored, centre, scale):
    """y, the iterate u_cur and a direction w0 that the candidates scale (candidate())"""
    n, p = xd.shape
    y = (rng.random(n) < 0.5).astype(np.float64)
    u_cur = np.concatenate([0.1 * rng.standard_normal(p) * (rng.random(p) < 0.7), [0.2]])
    w0 = rng.standard_normal(p)
    return SimpleNamespace(x=x, xd=xd, stored=stored, sparse=sp.issparse(x), centre=bool(centre), scale=scale, y=y, u_cur=u_cur,
                           w0=w0, n=n, p=p)


def candidate(case, kind):
    """(w, b): zero with b0 = 0.3; else w0 scaled so that the largest |eta| over the samples is CANDIDATES[kind] (about 3;
    about 40: the dynamic range of v and the cancellation in r; 800: exp overflows on the rows beyond 709.78 and
    underflows to 0 on those below -745)."""
    target = CANDIDATES[kind]
    if target == 0.0:
        return np.concatenate([np.zeros(case.p), [0.3]])
    mean = case.xd.sum(axis=0) / case.n if case.centre else np.zeros(case.p)
    eta0 = (case.xd - mean) @ (case.w0 / case.scale)
    top = np.abs(eta0).max()
    w = case.w0 * (target / top) if top > 0 else case.w0
    return np.concatenate([w, [0.0 if kind == "overflow" else 0.1]])


# penalties of the inner solve: (name, l2, l1, ridge) for mix in {0, 0.5, 1} at lambda = 0.05
PENALTIES = [("mix0_ridge", 0.05, 0.0, True), ("mix0.5", 0.025, 0.025, False), ("mix1", 0.0, 0.05, False)]


# ---------------------------------------------------------------------------------------------------------------
# the checks: what sgdnet_amd.diagnostics.newton_probe returns (GPU), or restate() below (CPU), against the above
# ---------------------------------------------------------------------------------------------------------------

def inside(got, ref, what, mask=None):
    """|got - ref.v| <= ref.e wherever mask holds; prints the entry closest to (or farthest beyond) its bound"""
    got = np.asarray(got, dtype=LD)
    assert got.shape == np.shape(ref.v), f"{what}: shape {got.shape}"
    mask = np.ones(got.shape, dtype=bool) if mask is None else mask
    assert not np.any(np.isnan(got[mask])), f"{what}: NaN"
    err, bound = np.abs(got - ref.v)[mask], np.broadcast_to(ref.e, got.shape)[mask]
    if err.size == 0:
        return
    worst = int(np.argmax(err - bound))
    print(f"{what}: closest to its bound: error {float(err[worst]):.3e}, bound {float(bound[worst]):.3e}")
    assert np.all(err <= bound), f"{what}: error {float(err[worst]):.3e} outside the bound {float(bound[worst]):.3e}"


def check_candidate(u_out, a_out, rec, u_want, u_cur, scale, what):
    """a published candidate: u bitwise, a = u / scale bitwise (one IEEE division), the record of publish_candidate"""
    ref = record_reference(u_out, u_cur, scale)
    if u_want is not None:
        assert np.array_equal(u_out, u_want), f"{what}: u"
    assert np.array_equal(a_out, ref.a), f"{what}: a is not u / scale"
    assert rec["change"] == ref.change and rec["size"] == ref.size, f"{what}: change / size are not the exact maxima"
    inside(rec["half_sq"], ref.half_sq, f"{what}: half_sq")
    inside(rec["abs"], ref.abs, f"{what}: abs")


def check_publish(o, case, u, t):
    check_candidate(o.pub_u, o.pub_a, o.pub_rec, np.asarray(u, dtype=np.float64), case.u_cur, case.scale, "publish")
    want = blend_f64(case.u_cur, u, t)
    if t == 1.0 or np.frexp(t)[0] == 0.5:            # t (u - u_cur) is exact: the same bits with or without a fused multiply-add
        check_candidate(o.blend_u, o.blend_a, o.blend_rec, want, case.u_cur, case.scale, "blend")
    else:
        diff = np.abs(t * (np.asarray(u) - case.u_cur))
        inside(o.blend_u, Val(want.astype(LD), 3 * U * (np.abs(case.u_cur) + diff)), "blend: u")
        check_candidate(o.blend_u, o.blend_a, o.blend_rec, None, case.u_cur, case.scale, "blend")


def check_mean(o, case):
    inside(o.mean, mean_reference(case.xd, case.stored, case.centre), "mean")
    if not case.centre:
        assert np.all(o.mean == 0.0), "mean: not exactly 0 without centring"


def check_state(o, case):
    """the state pass at a = o.pub_a with the means o.mean"""
    ref = state_reference(case.xd, o.mean, o.pub_a, case.y)
    inside(o.v, ref.v, "state: v")
    inside(o.r, ref.r, "state: r")
    assert np.all(o.v[ref.overflow] == 0.0), "state: v is not exactly 0 where exp overflows"
    if ref.overflow.any():
        assert o.loss == np.inf, f"state: loss {o.loss}, the reference says inf"
    else:
        assert np.isfinite(o.loss), f"state: loss {o.loss}, the reference is finite"
        inside(o.loss, ref.loss, "state: loss")
    inside(o.V, sum_reference(o.v), "state: V")
    inside(o.R, sum_reference(o.r), "state: R")
    return ref


def check_moments(o, case):
    """the moments pass from the returned mean, v, r, V and R"""
    if case.sparse:
        ref = sparse_moment_reference(case.xd, case.stored, o.mean, o.v, o.r, o.V, o.R)
    else:
        ref = dense_moment_reference(case.xd, o.mean, o.v, o.r)
    inside(o.M, ref, "moments: M", upper(case.p + 2))
    return ref


def check_inner(o, case, l2, l1, ridge, fit_intercept, max_sweeps, tol):
    """the inner solve on the returned M about u_cur"""
    p = case.p
    rec, u = o.cd_rec, o.cd_u
    check_candidate(o.cd_u, o.cd_a, rec, None, case.u_cur, case.scale, "inner")
    sweeps = int(rec["sweeps"])
    assert rec["sweeps"] == sweeps and 1 <= sweeps <= max_sweeps, f"inner: {rec['sweeps']} sweeps of at most {max_sweeps}"
    conv, negl = rec["converged"], rec["negligible"]
    assert conv in (0.0, 1.0) and negl in (0.0, 1.0) and (conv or not negl), f"inner: flags {conv}, {negl}"
    assert conv or sweeps == max_sweeps, "inner: stopped early without converging"
    H, q = model_from_M(o.M, case.scale, case.n)
    res, bound, visited = optimality(u, case.u_cur, H, q, l2, l1, ridge, fit_intercept, tol, sweeps)
    pen = np.arange(p + 1) < p
    assert np.all(u[pen & ~visited] == 0.0), "inner: a penalised coordinate without curvature or penalty must go to 0"
    if not fit_intercept or not visited[p]:
        assert u[p] == case.u_cur[p], "inner: the intercept moved"
    eta_sq = (np.asarray(u, dtype=LD) ** 2 * np.diag(H))[pen | bool(fit_intercept)].max()
    lim = LD(NEGLIGIBLE) ** 2
    assert (eta_sq <= lim * (1 + 16 * U)) if negl else (eta_sq >= lim * (1 - 16 * U)), f"inner: negligible = {negl} at {float(eta_sq):.3e}"
    if conv and not negl:
        k = int(np.argmax(np.where(visited, res - bound, -np.inf)))
        print(f"inner: {sweeps} sweeps, largest optimality residual {float(res[visited].max()):.3e}, bound at the worst {float(bound[k]):.3e}")
        assert np.all(res[visited] <= bound[visited]), f"inner: coordinate {k} misses optimality by {float(res[k]):.3e}, bound {float(bound[k]):.3e}"
    if sweeps == 1:
        inside(u, single_sweep_reference(o.M, case.scale, case.n, case.u_cur, l2, l1, ridge, fit_intercept), "inner: single sweep")
        f64 = sweeps_f64(o.M, case.scale, case.n, case.u_cur, l2, l1, ridge, fit_intercept, 1, tol)[0]
        one = single_sweep_reference(o.M, case.scale, case.n, case.u_cur, l2, l1, ridge, fit_intercept)
        inside(u, Val(f64.astype(LD), 2 * one.e), "inner: single sweep against float64 numpy")


def check_probe(o, case, u, t, l2, l1, ridge, fit_intercept=True, max_sweeps=1000, tol=1e-7):
    check_mean(o, case)
    check_publish(o, case, u, t)
    check_state(o, case)
    check_moments(o, case)
    check_inner(o, case, l2, l1, ridge, fit_intercept, max_sweeps, tol)


def restate(case, u, t, l2, l1, ridge, fit_intercept=True, max_sweeps=1000, tol=1e-7, fsum=seq_sum, wrong=None):
    """One outer step in float64, every sum through fsum: the fields of sgdnet_amd.diagnostics.newton_probe"""
    u = np.asarray(u, dtype=np.float64)
    p = case.p
    o = SimpleNamespace(mean=mean_f64(case.xd, case.stored, case.centre, fsum))

    def published(un):
        h, a = record_f64(un, fsum)
        return (un, np.concatenate([un[:p] / case.scale, un[p:]]),
                dict(half_sq=h, abs=a, change=float(np.abs(un - case.u_cur).max()), size=float(np.abs(un).max())))

    o.pub_u, o.pub_a, o.pub_rec = published(u.copy())
    o.blend_u, o.blend_a, o.blend_rec = published(blend_f64(case.u_cur, u, t))
    s = state_f64(case.xd, case.stored, case.centre, o.mean, o.pub_a, case.y, fsum, wrong)
    o.v, o.r, o.loss, o.V, o.R = s.v, s.r, s.loss, s.V, s.R
    if case.sparse:
        o.M = sparse_moments_f64(case.xd, case.stored, o.mean, o.v, o.r, o.V, o.R, fsum, wrong)
    else:
        o.M = dense_moments_f64(case.xd, o.mean, o.v, o.r, fsum, wrong)
    uc, sweeps, conv, negl = sweeps_f64(o.M, case.scale, case.n, case.u_cur, l2, l1, ridge, fit_intercept, max_sweeps, tol, wrong)
    o.cd_u, o.cd_a, rec = published(uc)
    o.cd_rec = dict(rec, loss=o.loss, sweeps=float(sweeps), converged=float(conv), negligible=float(negl))
    return o

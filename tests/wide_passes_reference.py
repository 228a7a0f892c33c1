"""Pure-numpy reference of what the wide Newton modes add to one outer step (sgdnet_amd/csrc/newton.hip: wnewton,
sgdnet_amd/csrc/mnewton.hip: wmnewton, sgdnet_amd/csrc/wide_cd_device.hpp), shared by tests/test_wide_passes_reference.py
(CPU) and tests/test_gpu_wnewton_passes.py / tests/test_gpu_wmnewton_passes.py (GPU).  The mean, the publish, the state pass
and the moments are the narrow modes' kernels on other grids: their truths, bounds and float64 restatements are those of
tests/newton_reference.py (N) and tests/mnewton_reference.py (MN), imported, not copied.  This file adds the scale pass,
the list solve and the inputs.  No tolerance in it comes from what a device returned.

Layout.  `count` coordinates: P = p + 1 (wnewton; the intercept is coordinate p) or Q = K (p + 1) (wmnewton; coordinate
(k, a) at k (p + 1) + a, a = p the intercept of class k).  ld = count rounded up to 16.  The matrix is kept as the probes
return it: an array (count, ld) whose ROW j is COLUMN j of the kernel's matrix, A[j, k] = H[k + ld j]; the columns
count .. ld - 1 of the array are the kernel's zero pad rows.

Scale pass (wide_scale_kernel, mnewton_wide_scale_kernel), bitwise.  Every entry is formed from one entry of the returned
M by two IEEE divisions and one IEEE product (the library is built without contraction):
    wnewton    H[k, j] = M[min(j, k), max(j, k)] / n / (s_j s_k),            q[j] = M[j, p + 1] / n / s_j,
    wmnewton   H[(k, a), (l, b)] = M[pair(min(k, l), max(k, l))][min(a, b), max(a, b)] / n / (s_a s_b),
               q[(k, a)] = M[pair(k, k)][a, p + 1] / n / s_a       (the class pair in ascending order on EITHER side of the
               diagonal, the feature pair likewise: mnewton_wide_scale_kernel's comment),
    s = scale for the features and 1 for an intercept, Hd[j] = H[j, j].  numpy's float64 division and product are the same
    IEEE operations, and a product of two doubles commutes bitwise, so the restatement equals the device bit for bit.
    Checked besides: ld, H bitwise symmetric, the pad exactly 0.0 (+0.0: the bytes) in every column.

List solve (newton_wide_cd_kernel, mnewton_wide_cd_kernel), restated in float64 and long double (list_solve):
    start     u = u_cur, g = -q exactly; the list is {penalised j : u_j != 0} and the intercept(s) when they are fitted.
    screen    every penalised j outside the list: the coordinate update from u_j = 0 with the current g; those whose
              result is not 0 join; the list stays ascending.
    sweep     the coordinate update (newton_coord_new_u / mnewton_coord_new_u) over the list in ascending order; a
              coordinate that moves by d does g[k] += H[k, j] d for ALL k (one fused multiply-add on the device, a product
              and a sum here: the drift term below allows two roundings).  A sweep ends with the narrow kernels' rule over
              the coordinates of the list (all zero, or max|d| / max|nu| <= tol, or negligible).
    re-screen when a sweep met the rule; the solve has converged when the screen adds nothing.  max_sweeps counts the list
              sweeps across the screens; a solve that runs out of them stops with converged = 0 (after a screen that added
              coordinates no sweep may be left: then negligible can be 1 with converged = 0, the last sweep's flag).

  Why N.optimality / MN.optimality's bound B_j = conv_j + drift_j + local_j (+ zero_j) holds for the list algorithm, for
  the model (H, q) the scale kernel RETURNED (float64 words taken as exact: nothing is rounded between model and kernel, so
  the part of local_j that pays for the narrow kernels' prologue is slack here), when the record says converged and not
  merely negligible:
    The solve ended with a list sweep that met the rule, followed by a screen that added nothing; nothing moved after
    that sweep.
    j outside the list   is penalised, was never in the list, so u_j = u_cur_j = 0 bitwise, and the last screen computed the
              update from 0 with the RUNNING g_j and got 0: z = 0 H_jj - g_j = -g_j exactly, so |g_j(running)| <= l1 (under
              the mnewton rule: or the thresholded step is negligible, which zero_j pays for; under ridge: g_j(running) = 0,
              or a quotient that underflows).  The running g_j is the true gradient but for the rounding of its updates:
              drift_j.  conv_j is not needed (slack).
    j in the list         when j was set in the last sweep its condition held for the running g_j but for the update's own
              rounding (local_j); the coordinates of the list set after it moved by at most tol max|nu| <= tol max|u| each
              (the rule's maxima run over the list; every coordinate outside it is 0 or a frozen intercept, which only
              raises max|u|), shifting g_j by at most sum_(k != j) |H_jk| tol max|u| = conv_j.  The screen that followed
              changes no g.
    drift_j   g_j is updated once per MOVE: at most (list length) <= count times a sweep, `sweeps` list sweeps in all, each
              update one or two roundings of at most u (|H_jk d| + |g_j|) <= 2 u S_j while the iterates stay within D of
              u_cur (the assumption N's docstring states).  g starts as -q exactly.  So 2 u sweeps count S_j stands, with
              `sweeps` the record's count of list sweeps.
    A coordinate the list lost (never screened in, or dropped from the list while away from its optimum) has a residual of
    the order of its gradient, not of u: this is the check that sees it.  max(|g_j| - l1, 0) at zeros is over ALL
    coordinates, whether the kernel visited them or not.
  Single sweep (max_sweeps = 1), list_single_sweep_reference: the first screen's list is decided from exact words
    (z = q_j; "moves from 0" iff |q_j| > l1, under ridge iff q_j != 0) -- an input whose |q_j| is within 1e-9 relative of l1
    is refused (asserted) -- and under the mnewton rule a thresholded step from 0 that is negligible does not join (an
    input within 1e-6 relative of that threshold is refused too).  Then ONE sweep over that list in long double with the error
    propagation of N.single_sweep_reference (E_H = 0, E_g starts at 0: the model is exact).  A full narrow sweep would also
    move the coordinates the first screen left out; the list sweep does not.
  Record: N.check_candidate / MN.check_candidate as they are (the wide publish is the narrow one by the first wavefront; at
    most ceil(count / 64) terms per lane: the sums' depth is taken for the count at hand).
"""
from types import SimpleNamespace

import numpy as np

import mnewton_reference as MN
import newton_reference as N
from newton_reference import NEGLIGIBLE, PENALTIES, SUMS, _soft, inside, seq_sum
from setup_reference import LD, U, Val, fl_mul, fl_sub, fl_sum, gamma

__all__ = ["PENALTIES", "SUMS", "seq_sum", "inside"]

WNEWTON_MAX_FEATURES = 5819                 # csrc/newton.hpp: kWnewtonMaxFeatures (the GPU test asserts the library agrees)
WMNEWTON_MAX_COORDINATES = 5820             # csrc/mnewton.hpp: kWmnewtonMaxCoordinates


def leading_dim(count):
    return (count + 15) // 16 * 16


def wide_row_chunks(n, ncols, class_pairs=1):
    """csrc/wide_layout.hpp: wide_row_chunks; csrc/mnewton.hpp: wmnewton_row_chunks with the class pairs"""
    t = (ncols + 15) // 16
    wg = t * (t + 1) // 2 * class_pairs
    cap = 1 if wg >= 1024 else 1024 // wg
    return max(1, min((n + 255) // 256, cap))


def wide_width(count_or_p):
    """csrc/wide_layout.hpp: wide_cd_width (wnewton passes p, wmnewton Q)"""
    return 256 if count_or_p <= 512 else 1024


# ---------------------------------------------------------------------------------------------------------------
# the two modes: how a flat coordinate is penalised and updated, and how the model comes out of M
# ---------------------------------------------------------------------------------------------------------------

def _sym_block(Mb, P, F, wrong):
    """the P x P moment block with the entry below the diagonal taken from the upper triangle ("wrong_triangle": from where
    it stands, which nothing defines)"""
    Mb = np.asarray(Mb, dtype=F)[:P, :P]
    if wrong == "wrong_triangle":
        return Mb.T.copy()                     # entry [row k, col j] of the result = M[j, k], as stored, for all j, k
    up = np.triu(Mb)
    return up + np.triu(Mb, 1).T


def wn_scale_f64(M, scale, n, wrong=None, dtype=np.float64):
    """wide_scale_kernel.  wrong: "no_1_over_n", "s_j_squared" (H_kj / s_j^2), "wrong_triangle", "q_from_ones", "pad_nonzero".
    Returns A (P, ld) -- row j is column j --, Hd, q."""
    F = dtype
    nc = M.shape[0]
    p, P = nc - 2, nc - 1
    ld = leading_dim(P)
    s = np.concatenate([np.asarray(scale, dtype=F), [F(1)]])
    A = np.zeros((P, ld), dtype=F)
    sym = _sym_block(M, P, F, wrong)
    if wrong != "no_1_over_n":
        sym /= F(n)
    sym /= (s[:, None] * s[:, None]) if wrong == "s_j_squared" else (s[:, None] * s[None, :])
    A[:, :P] = sym
    del sym
    q = np.asarray(M, dtype=F)[:P, p if wrong == "q_from_ones" else p + 1] / F(n) / s
    if wrong == "pad_nonzero" and ld > P:
        A[0, P] = F(1e-300)
    return A, np.diagonal(A).copy(), q


def wmn_scale_f64(M, scale, n, K, wrong=None, dtype=np.float64):
    """mnewton_wide_scale_kernel.  wrong: those of wn_scale_f64 and "pair_not_reordered" (below the diagonal the class pair
    (l, k), l > k, is looked up as it stands: the row-by-row index formula with its arguments the wrong way round)."""
    F = dtype
    nc = M.shape[1]
    p, P = nc - 2, nc - 1
    Q = K * P
    ld = leading_dim(Q)
    pairs = M.shape[0]
    s = np.concatenate([np.asarray(scale, dtype=F), [F(1)]])
    ss = (s[:, None] * s[:, None]) if wrong == "s_j_squared" else (s[:, None] * s[None, :])
    A = np.zeros((Q, ld), dtype=F)
    blocks = {}
    for k in range(K):
        for l in range(K):
            lo, hi = (k, l) if k <= l else (l, k)
            idx = MN.pair_index(lo, hi, K)
            if wrong == "pair_not_reordered" and k > l:
                idx = MN.pair_index(k, l, K) % pairs
            if idx not in blocks:
                b = _sym_block(M[idx], P, F, wrong)
                if wrong != "no_1_over_n":
                    b /= F(n)
                b /= ss
                blocks[idx] = b
            # column c2 = (l, b), entry c1 = (k, a): row c2 of the array
            A[l * P:(l + 1) * P, k * P:(k + 1) * P] = blocks[idx]
    Mf = np.asarray(M)
    q = np.concatenate([np.asarray(Mf[MN.pair_index(k, k, K), :P, p if wrong == "q_from_ones" else p + 1], dtype=F) / F(n) / s
                        for k in range(K)])
    if wrong == "pad_nonzero" and ld > Q:
        A[0, Q] = F(1e-300)
    return A, np.diagonal(A).copy(), q


def check_scale(o, want, count):
    """what the scale kernel wrote against the restatement from the returned M: all bitwise"""
    A, Hd, q = want
    ld = leading_dim(count)
    assert o.ld == ld and o.H.shape == (count, ld), f"scale: ld {o.ld}, H {o.H.shape}; the count {count} rounds up to {ld}"
    pad = o.H[:, count:]
    assert pad.tobytes() == bytes(pad.nbytes), "scale: the pad rows are not exactly 0.0 in every column"
    sq = o.H[:, :count]
    assert not np.any(np.isnan(sq)), "scale: H has a NaN"
    assert np.array_equal(sq, sq.T), "scale: H is not bitwise symmetric"
    assert np.array_equal(sq, A[:, :count]), "scale: H is not M / n / (s s') in the kernel's order of operations"
    assert np.array_equal(o.Hd, np.diagonal(sq)) and np.array_equal(o.Hd, Hd), "scale: Hd is not the diagonal of H"
    assert np.array_equal(o.q, q), "scale: q is not M[., last] / n / s"
    print(f"scale: {count} x {count} entries, {ld - count} pad rows, diag H and q bitwise")


def narrow_prologue_wn(M, scale, n):
    """newton_cd_solve's prologue on the same M, in float64: the packed triangle as a full matrix, and q"""
    A, _Hd, q = wn_scale_f64(M, scale, n)
    P = M.shape[0] - 1
    return A[:, :P], q


def narrow_prologue_wmn(M, scale, n, K):
    """mnewton_cd_solve's prologue on the same M, in float64 (MN.joint_model in the kernel's order of operations)"""
    return MN.joint_model(M, scale, n, K, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------
# the list solve
# ---------------------------------------------------------------------------------------------------------------

def coord_new_u(rule, hjj, uj, gj, al, be, ridge, pen, lim):
    """newton_coord_new_u (rule "newton") / mnewton_coord_new_u (rule "mnewton") in the type of its arguments"""
    z = hjj * uj - gj
    den = hjj + al if pen else hjj
    nu = _soft(z, be) if (pen and not ridge) else z
    if rule == "newton":
        return nu / den if den > 0 else (uj * 0 if pen else uj)
    nu = nu / den if den > 0 else uj
    with np.errstate(over="ignore"):
        if pen and not ridge and den > 0 and nu * nu * hjj <= lim:
            nu = uj * 0
    return nu


def list_solve(A, q, pen, u_cur, l2, l1, ridge, fit_intercept, max_sweeps, tol, rule, wrong=None, dtype=np.float64):
    """The wide inner solve on the model (A, q): A (count, >= count), row j the column j the kernel reads when j moves.
    wrong: "no_rescreen" (done when the first list has converged), "no_intercept_in_list", "no_screen" (the list is the
    start's), "high_word_lost" (at a re-screen the membership of the coordinates 32 .. 63 of every 64 is forgotten: they
    stay only if they would move from 0), "odd_last_not_moved" (an odd count: the column move leaves the last g alone).
    Returns u, sweeps, converged, negligible, screens, added (per screen: how many coordinates it added), listed (every
    coordinate that ever was in the list)."""
    F = dtype
    count = len(q)
    Hc = np.asarray(A, dtype=F)[:, :count]
    hd = np.diagonal(Hc).copy()
    g = -np.asarray(q, dtype=F)
    u = np.asarray(u_cur, dtype=F).copy()
    al, be = F(l2), F(0 if ridge else l1)
    lim = F(NEGLIGIBLE) * F(NEGLIGIBLE)
    pen = np.asarray(pen, dtype=bool)
    member = np.where(pen, u != 0, bool(fit_intercept) and wrong != "no_intercept_in_list")
    listed = member.copy()
    moved_cols = count - 1 if (wrong == "odd_last_not_moved" and count % 2 == 1) else count
    sweeps, converged, negligible, screens, added = 0, False, False, 0, []
    n_list = int(member.sum())
    while True:
        old = member
        if wrong == "high_word_lost" and screens > 0:
            old = member & ~(pen & (np.arange(count) % 64 >= 32))
        new = old.copy()
        if wrong != "no_screen":
            for j in np.flatnonzero(pen & ~old):
                if coord_new_u(rule, hd[j], F(0), g[j], al, be, ridge, True, lim) != 0:
                    new[j] = True
        n_new = int(new.sum())
        added.append(int((new & ~member).sum()))
        if screens > 0 and (n_new == n_list or wrong == "no_rescreen"):
            converged = True
            break
        screens += 1
        member, n_list = new, n_new
        listed = listed | member
        order = np.flatnonzero(member)
        met = False
        while sweeps < max_sweeps and not met:
            change = size = eta_sq = F(0)
            for j in order:
                uj, hjj = u[j], hd[j]
                nu = coord_new_u(rule, hjj, uj, g[j], al, be, ridge, bool(pen[j]), lim)
                d = nu - uj
                with np.errstate(over="ignore"):
                    change, size, eta_sq = max(change, abs(d)), max(size, abs(nu)), max(eta_sq, nu * nu * hjj)
                if d != 0:
                    u[j] = nu
                    g[:moved_cols] = g[:moved_cols] + Hc[j, :moved_cols] * d
            sweeps += 1
            negligible = bool(eta_sq <= lim)
            met = bool((size == 0 and change == 0) or (size != 0 and change / size <= tol) or negligible)
        if not met:
            break
        if wrong == "no_screen":
            converged = True
            break
    return SimpleNamespace(u=u, sweeps=sweeps, converged=converged, negligible=negligible, screens=screens, added=added, listed=listed)


def first_list(hd, q, pen, u_cur, l2, l1, ridge, fit_intercept, rule):
    """the list of the first sweep, from exact words; refuses (asserts) an input on the edge of a decision (module docstring)"""
    hd, q, u_cur = (np.asarray(a, dtype=np.float64) for a in (hd, q, u_cur))
    be = 0.0 if ridge else float(l1)
    member = np.where(pen, u_cur != 0, bool(fit_intercept))
    out = pen & ~member
    assert np.all(np.abs(np.abs(q[out]) - be) > 1e-9 * max(be, 1e-300)) or be == 0.0, "a |q_j| on the edge of the first screen's threshold"
    den = hd + l2
    with np.errstate(divide="ignore", invalid="ignore"):
        step = np.where(den > 0, (q if ridge else np.sign(q) * np.maximum(np.abs(q) - be, 0)) / np.where(den > 0, den, 1), 0.0)
    if rule == "mnewton" and not ridge:
        eta = np.abs(step) * np.sqrt(np.maximum(hd, 0))
        edge = out & (step != 0) & (np.abs(eta - NEGLIGIBLE) <= 1e-6 * NEGLIGIBLE)
        assert not edge.any(), "a screened step on the edge of the exact-zero rule"
        step = np.where(eta * eta <= NEGLIGIBLE * NEGLIGIBLE, 0.0, step)
    return member | (out & (step != 0))


def list_single_sweep_reference(A, q, pen, u_cur, l2, l1, ridge, fit_intercept, rule):
    """One sweep over the first screen's list in long double on the returned model, and the propagated bound E on a
    computed sweep's u (Val).  Coordinates outside the list stay: bound 0."""
    count = len(q)
    H = np.asarray(A, dtype=LD)[:, :count]
    ql = np.asarray(q, dtype=LD)
    member = first_list(np.diagonal(np.asarray(A)[:, :count]), q, pen, u_cur, l2, l1, ridge, fit_intercept, rule)
    g, Eg = -ql.copy(), np.zeros(count, dtype=LD)
    u = np.asarray(u_cur, dtype=LD).copy()
    Eu = np.zeros(count, dtype=LD)
    al, be = LD(l2), LD(0 if ridge else l1)
    for j in np.flatnonzero(member):
        pj = bool(pen[j])
        uj, hjj = u[j], H[j, j]
        z = hjj * uj - g[j]
        den = hjj + al if pj else hjj
        Ez = Eg[j] + U * (abs(hjj * uj) + abs(z))
        sz = _soft(z, be) if (pj and not ridge) else z
        if den > 0:
            Eden = U * den
            nu = sz / den
            Enu = (Ez + U * abs(sz) + abs(nu) * Eden) / (den - Eden) + U * abs(nu)
            if rule == "mnewton" and pj and not ridge:
                if hjj > 0 and (abs(nu) - Enu) * np.sqrt(hjj) <= LD(NEGLIGIBLE) * (1 + 8 * U):
                    Enu = Enu + abs(nu)                      # the exact zero of the kernel: either side of its threshold
                    if nu * nu * hjj <= LD(NEGLIGIBLE) ** 2:
                        nu = LD(0)
                elif hjj <= 0:
                    nu = LD(0)
        else:
            nu, Enu = ((LD(0) if pj else uj) if rule == "newton" else uj), LD(0)
        d = nu - uj
        Ed = Enu + U * abs(d)
        u[j], Eu[j] = nu, Enu
        upd = H[j, :] * d
        g = g + upd
        Eg = Eg + np.abs(H[j, :]) * Ed + U * np.abs(upd) + U * (np.abs(g) + Eg)
    return Val(u, LD(1.01) * Eu), member


def _optimality(mode, u, u_cur, H, q, pen, l2, l1, ridge, fit_intercept, tol, sweeps):
    """N.optimality / MN.optimality on the returned model: (residual, bound, visited, forced, stays)"""
    if mode == "wnewton":
        res, bound, visited = N.optimality(u, u_cur, H, q, l2, l1, ridge, fit_intercept, tol, sweeps)
        return res, bound, visited, pen & ~visited, ~pen & ~visited     # without curvature or penalty: to 0; the intercept: stays
    res, bound, visited, forced = MN.optimality(u, u_cur, H, q, pen, l2, l1, ridge, fit_intercept, tol, sweeps)
    return res, bound, visited, forced, ~visited & ~forced


def check_list_solve(o, mode, pen, u_cur, l2, l1, ridge, fit_intercept, max_sweeps, tol, must_converge=False):
    """the inner solve on the RETURNED H and q about u_cur; the candidate's record is checked by the caller"""
    count = len(o.q)
    rec, u = o.cd_rec, np.asarray(o.cd_u)
    u_cur = np.asarray(u_cur, dtype=np.float64)
    sweeps = int(rec["sweeps"])
    assert rec["sweeps"] == sweeps and 1 <= sweeps <= max_sweeps, f"inner: {rec['sweeps']} sweeps of at most {max_sweeps}"
    conv, negl = rec["converged"], rec["negligible"]
    assert conv in (0.0, 1.0) and negl in (0.0, 1.0), f"inner: flags {conv}, {negl}"
    assert conv or sweeps == max_sweeps, "inner: stopped early without converging"
    if must_converge:
        assert conv == 1.0, f"inner: not converged after {sweeps} sweeps"
    H = np.asarray(o.H, dtype=LD)[:, :count]
    q = np.asarray(o.q, dtype=LD)
    res, bound, visited, forced, stays = _optimality(mode, u, u_cur, H, q, pen, l2, l1, ridge, fit_intercept, tol, sweeps)
    assert np.all(u[forced] == 0.0), "inner: a penalised coordinate without curvature that the update sends to 0 is not 0.0"
    assert u[stays].tobytes() == u_cur[stays].tobytes(), "inner: a coordinate that is not visited, or stays by its rule, moved"
    if not fit_intercept:
        assert u[~pen].tobytes() == u_cur[~pen].tobytes(), "inner: a frozen intercept moved"
    seen = pen | bool(fit_intercept)
    eta_sq = (np.asarray(u, dtype=LD) ** 2 * np.diagonal(H))[seen].max() if seen.any() else LD(0)
    lim = LD(NEGLIGIBLE) ** 2
    assert (eta_sq <= lim * (1 + 16 * U)) if negl else (eta_sq >= lim * (1 - 16 * U)), f"inner: negligible = {negl} at {float(eta_sq):.3e}"
    if conv and not negl and visited.any():
        k = int(np.argmax(np.where(visited, res - bound, -np.inf)))
        ratio = float(np.max(np.where(visited & (bound > 0), res / np.where(bound > 0, bound, 1), 0)))
        print(f"inner: {sweeps} sweeps, largest optimality residual {float(res[visited].max()):.3e}, bound at the worst {float(bound[k]):.3e}, "
              f"largest residual / bound {ratio:.3f}")
        assert np.all(res[visited] <= bound[visited]), f"inner: coordinate {k} misses optimality by {float(res[k]):.3e}, bound {float(bound[k]):.3e}"
    if max_sweeps == 1:
        rule = "newton" if mode == "wnewton" else "mnewton"
        one, member = list_single_sweep_reference(o.H, o.q, pen, u_cur, l2, l1, ridge, fit_intercept, rule)
        assert u[~member].tobytes() == u_cur[~member].tobytes(), "inner: single sweep: a coordinate outside the first list moved"
        inside(u, one, "inner: single sweep")
        f64 = list_solve(o.H, o.q, pen, u_cur, l2, l1, ridge, fit_intercept, 1, tol, rule).u
        inside(u, Val(f64.astype(LD), 2 * one.e), "inner: single sweep against float64 numpy")
        if fit_intercept and conv:            # one sweep from u_cur: the sweep's own maxima are the record's
            ch, sz = rec["change"], rec["size"]
            assert (sz == 0 and ch == 0) or (sz != 0 and ch / sz <= tol) or bool(negl), f"inner: converged with change {ch}, size {sz}"


# ---------------------------------------------------------------------------------------------------------------
# the moments at the limit: a fixed sample of entries
# ---------------------------------------------------------------------------------------------------------------

def sample_positions(nc, rows, seed, extra=4000):
    """(a, b), a <= b, a < rows: the corners, the edges of the last 16-column tile and `extra` seeded positions"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, rows, extra)
    b = rng.integers(0, nc, extra)
    a, b = np.minimum(a, b), np.maximum(a, b)
    last = (nc - 1) // 16 * 16
    edge = [0, 1, 15, 16, 17, last - 1, last, last + 1, rows - 2, rows - 1, nc - 2, nc - 1]
    ea, eb = np.meshgrid(edge, edge, indexing="ij")
    a, b = np.concatenate([a, ea.ravel()]), np.concatenate([b, eb.ravel()])
    keep = (a >= 0) & (b >= 0) & (a <= b) & (a < rows) & (b < nc)
    return a[keep], b[keep]


def _dev_cols(xd, mean):
    n, p = xd.shape
    d = fl_sub(Val(xd.astype(LD)), Val(np.asarray(mean, dtype=LD)[None, :] + np.zeros((n, 1), dtype=LD)))
    return Val(np.concatenate([d.v, np.ones((n, 1), dtype=LD)], axis=1), np.concatenate([d.e, np.zeros((n, 1), dtype=LD)], axis=1))


def check_wn_moments_sampled(o, case, seed=1):
    """N.dense_moment_reference's entries at sample_positions only (34 million entries in long double would take minutes)"""
    n, p = case.xd.shape
    a, b = sample_positions(p + 2, p + 1, seed)
    A = _dev_cols(case.xd, o.mean)                                    # [d | 1]
    v, r = np.asarray(o.v, dtype=LD), np.asarray(o.r, dtype=LD)
    Ab = Val(A.v[:, np.minimum(b, p)], A.e[:, np.minimum(b, p)])
    B = fl_mul(Val(v[:, None] + np.zeros((1, len(b)), dtype=LD)), Ab)   # v d_b, v 1 (exact: the device stages v itself)
    is_d = (b < p)[None, :]
    B = Val(np.where(b[None, :] == p + 1, r[:, None], B.v), np.where(is_d, B.e, 0))
    ref = fl_sum(fl_mul(Val(A.v[:, a], A.e[:, a]), B), np.ones((n, len(a)), dtype=bool), 0)
    inside(o.M[a, b], ref, f"moments: M at {len(a)} sampled entries")


def check_wmn_moments_sampled(o, c, seed=1):
    """MN.moment_reference's entries at sample_positions only, for every class pair"""
    n, p = c.xd.shape
    K = c.K
    A = _dev_cols(c.xd, o.mean)
    mu = Val(np.asarray(o.mu, dtype=LD))
    yi = np.asarray(c.y).astype(int)
    one = Val(np.ones(n, dtype=LD))
    for i, (k, l) in enumerate(MN.pair_list(K)):
        a, b = sample_positions(p + 2, p + 1, seed + i)
        mk, ml = Val(mu.v[:, k], mu.e[:, k]), Val(mu.v[:, l], mu.e[:, l])
        if k == l:
            w = fl_mul(mk, fl_sub(one, mk))
            r = fl_sub(Val((yi == k).astype(LD)), mk)
        else:
            w = fl_mul(mk, ml)
            w, r = Val(-w.v, w.e), Val(np.zeros(n, dtype=LD))
        shape = (n, len(b))
        Ab = Val(A.v[:, np.minimum(b, p)], A.e[:, np.minimum(b, p)])
        wd = fl_mul(N._bro(Val(w.v[:, None], w.e[:, None]), shape), Ab)
        is_d = (b < p)[None, :]
        Bv = np.where(b[None, :] == p + 1, r.v[:, None], np.where(is_d, wd.v, w.v[:, None]))
        Be = np.where(b[None, :] == p + 1, r.e[:, None], np.where(is_d, wd.e, w.e[:, None]))
        ref = fl_sum(fl_mul(Val(A.v[:, a], A.e[:, a]), Val(Bv, Be)), np.ones(shape, dtype=bool), 0)
        got = o.M[i, a, b]
        if k != l:
            assert np.all(o.M[i, :p + 1, p + 1] == 0.0), f"moments: M: the q column of the off-diagonal pair ({k}, {l}) is not 0.0"
        inside(got, ref, f"moments: M of the pair ({k}, {l}) at {len(a)} sampled entries")


# ---------------------------------------------------------------------------------------------------------------
# whole probes: wnewton
# ---------------------------------------------------------------------------------------------------------------

def _depth_patch(count):
    """the record's sums at this count: ceil(count / 64) terms per lane in order, then the 6-step butterfly (N's 3 + 6 + 2
    at its 199 coordinates)"""
    return gamma(max((count + 63) // 64 - 1, 0) + 6 + 2)


def wn_pen(p):
    return np.arange(p + 1) < p


def wn_check_candidate(u_out, a_out, rec, u_want, u_cur, scale, what):
    """N.check_candidate with the sums' depth of this count (N's is written for at most 199 coordinates)"""
    u_out, u_cur = np.asarray(u_out, dtype=np.float64), np.asarray(u_cur, dtype=np.float64)
    p = len(u_out) - 1
    if u_want is not None:
        assert np.array_equal(u_out, u_want), f"{what}: u"
    a = np.concatenate([u_out[:p] / np.asarray(scale, dtype=np.float64), u_out[p:]])
    assert np.array_equal(a_out, a), f"{what}: a is not u / scale"
    assert rec["change"] == float(np.abs(u_out - u_cur).max()) and rec["size"] == float(np.abs(u_out).max()), \
        f"{what}: change / size are not the exact maxima"
    _check_sums(rec, u_out[:p], p + 1, what)


def _check_sums(rec, w, count, what):
    w = Val(np.asarray(w, dtype=LD))
    depth = _depth_patch(count)
    sq = fl_mul(w, w)
    inside(rec["half_sq"], Val(sq.v.sum() / 2, (sq.e.sum() + depth * (np.abs(sq.v) + sq.e).sum()) / 2), f"{what}: half_sq")
    inside(rec["abs"], Val(np.abs(w.v).sum(), depth * np.abs(w.v).sum()), f"{what}: abs")


def wmn_check_candidate(u_out, a_out, rec, u_want, c, what):
    u_out, u_cur = np.asarray(u_out, dtype=np.float64), np.asarray(c.u_cur, dtype=np.float64)
    pen = MN.penalised(c.K, c.p)
    if u_want is not None:
        assert np.array_equal(u_out, u_want), f"{what}: u"
    s = np.tile(np.concatenate([np.asarray(c.scale, dtype=np.float64), [1.0]]), c.K)
    assert np.array_equal(a_out, np.where(pen, u_out / s, u_out)), f"{what}: a is not u / scale"
    assert rec["change"] == float(np.abs(u_out - u_cur).max()) and rec["size"] == float(np.abs(u_out).max()), \
        f"{what}: change / size are not the exact maxima"
    _check_sums(rec, u_out[pen], c.Q, what)


def _check_publish(o, u_cur, u, t, cand):
    """publish at t = 1 bitwise; the blend bitwise at t = 1 and where t (u - u_cur) is exact, three roundings otherwise"""
    cand(o.pub_u, o.pub_a, o.pub_rec, np.asarray(u, dtype=np.float64), "publish")
    want = N.blend_f64(u_cur, u, t)
    if t == 1.0 or np.frexp(t)[0] == 0.5:
        cand(o.blend_u, o.blend_a, o.blend_rec, want, "blend")
    else:
        diff = np.abs(t * (np.asarray(u) - u_cur))
        inside(o.blend_u, Val(want.astype(LD), 3 * U * (np.abs(u_cur) + diff)), "blend: u")
        cand(o.blend_u, o.blend_a, o.blend_rec, None, "blend")


def fl_sum_long(t, mask, axis):
    """setup_reference.fl_sum without its limit of 4096 terms.  That limit is where the reference's OWN long-double sum stops
    being covered by the 2 in gamma(m + 2): a sum of k terms in long double errs by at most k 2^-64 = (k / 2048) u relative,
    which is 2 u at 4096.  Here the allowance grows with k: gamma(m + max(2, ceil(k / 2048))); up to 4096 terms the two agree."""
    own = max(2, -(-t.v.shape[axis] // 2048))
    m = int(mask.sum(axis=axis).max()) if mask.size else 0
    tv, te = np.where(mask, t.v, 0), np.where(mask, t.e, 0)
    return Val(tv.sum(axis=axis), te.sum(axis=axis) + gamma(m + own) * (np.abs(tv) + te).sum(axis=axis))


def wn_check_state(o, case):
    """N.check_state; beyond 4095 features (eta is a sum of p + 1 terms) with fl_sum_long in fl_sum's place for the call"""
    if case.p + 1 <= 4096:
        return N.check_state(o, case)
    kept, N.fl_sum = N.fl_sum, fl_sum_long
    try:
        return N.check_state(o, case)
    finally:
        N.fl_sum = kept


def wn_check_probe(o, case, u, t, l2, l1, ridge, fit_intercept=True, max_sweeps=1000, tol=1e-7, must_converge=False, sampled=False):
    """mean, publish, state and moments as N.check_probe holds them; then the scale pass (bitwise), the list solve on the
    returned H and q, the blend.  sampled: the moments on sample_positions only (the feature limit)."""
    def cand(uo, ao, rec, want, what):
        wn_check_candidate(uo, ao, rec, want, case.u_cur, case.scale, what)

    N.check_mean(o, case)
    _check_publish(o, case.u_cur, u, t, cand)
    wn_check_state(o, case)
    if sampled:
        check_wn_moments_sampled(o, case)
    else:
        N.check_moments(o, case)
    check_scale(o, wn_scale_f64(o.M, case.scale, case.n), case.p + 1)
    cand(o.cd_u, o.cd_a, o.cd_rec, None, "inner")
    check_list_solve(o, "wnewton", wn_pen(case.p), case.u_cur, l2, l1, ridge, fit_intercept, max_sweeps, tol, must_converge)


def _published_wn(un, case, fsum):
    h, a = N.record_f64(un, fsum)
    p = case.p
    return (un, np.concatenate([un[:p] / case.scale, un[p:]]),
            dict(half_sq=h, abs=a, change=float(np.abs(un - case.u_cur).max()), size=float(np.abs(un).max())))


SCALE_WRONG = ("no_1_over_n", "s_j_squared", "wrong_triangle", "q_from_ones", "pair_not_reordered", "pad_nonzero")
LIST_WRONG = ("no_rescreen", "no_intercept_in_list", "no_screen", "high_word_lost", "odd_last_not_moved")


def wn_restate(case, u, t, l2, l1, ridge, fit_intercept=True, max_sweeps=1000, tol=1e-7, fsum=seq_sum, wrong=None, upto=None):
    """One outer step of wnewton in float64, every any-order sum through fsum: the fields of diagnostics.wnewton_probe and
    `solve` (list_solve's own account).  upto = "scale": stop before the solve."""
    u = np.asarray(u, dtype=np.float64)
    o = SimpleNamespace(mean=N.mean_f64(case.xd, case.stored, case.centre, fsum))
    o.pub_u, o.pub_a, o.pub_rec = _published_wn(u.copy(), case, fsum)
    o.blend_u, o.blend_a, o.blend_rec = _published_wn(N.blend_f64(case.u_cur, u, t), case, fsum)
    s = N.state_f64(case.xd, case.stored, case.centre, o.mean, o.pub_a, case.y, fsum)
    o.v, o.r, o.loss, o.V, o.R = s.v, s.r, s.loss, s.V, s.R
    o.M = N.dense_moments_f64(case.xd, o.mean, o.v, o.r, fsum)
    o.H, o.Hd, o.q = wn_scale_f64(o.M, case.scale, case.n, wrong if wrong in SCALE_WRONG else None)
    o.ld = o.H.shape[1]
    if upto == "scale":
        return o
    o.solve = list_solve(o.H, o.q, wn_pen(case.p), case.u_cur, l2, l1, ridge, fit_intercept, max_sweeps, tol, "newton",
                         wrong if wrong in LIST_WRONG else None)
    o.cd_u, o.cd_a, rec = _published_wn(o.solve.u, case, fsum)
    o.cd_rec = dict(rec, loss=o.loss, sweeps=float(o.solve.sweeps), converged=float(o.solve.converged), negligible=float(o.solve.negligible))
    return o


# ---------------------------------------------------------------------------------------------------------------
# whole probes: wmnewton
# ---------------------------------------------------------------------------------------------------------------

def wmn_check_probe(o, c, u, t, l2, l1, ridge, fit_intercept=True, max_sweeps=1000, tol=1e-7, must_converge=False, sampled=False):
    def cand(uo, ao, rec, want, what):
        wmn_check_candidate(uo, ao, rec, want, c, what)

    MN.check_mean(o, c)
    _check_publish(o, c.u_cur, u, t, cand)
    MN.check_state(o, c)
    if sampled:
        check_wmn_moments_sampled(o, c)
    else:
        MN.check_moments(o, c)
    check_scale(o, wmn_scale_f64(o.M, c.scale, c.n, c.K), c.Q)
    cand(o.cd_u, o.cd_a, o.cd_rec, None, "inner")
    check_list_solve(o, "wmnewton", MN.penalised(c.K, c.p), c.u_cur, l2, l1, ridge, fit_intercept, max_sweeps, tol, must_converge)


def _published_wmn(un, c, fsum):
    pen = MN.penalised(c.K, c.p)
    s = np.tile(np.concatenate([c.scale, [1.0]]), c.K)
    h, a = MN.record_f64(un, c.K, fsum)
    return (un, np.where(pen, un / s, un), dict(half_sq=h, abs=a, change=float(np.abs(un - c.u_cur).max()), size=float(np.abs(un).max())))


def wmn_restate(c, u, t, l2, l1, ridge, fit_intercept=True, max_sweeps=1000, tol=1e-7, fsum=seq_sum, wrong=None, upto=None):
    """One outer step of wmnewton in float64: the fields of diagnostics.wmnewton_probe and `solve`"""
    u = np.asarray(u, dtype=np.float64)
    K, p = c.K, c.p
    o = SimpleNamespace(mean=np.array([fsum(c.xd[:, j]) / c.n if c.centre else 0.0 for j in range(p)]).reshape(p))
    o.pub_u, o.pub_a, o.pub_rec = _published_wmn(u.copy(), c, fsum)
    o.blend_u, o.blend_a, o.blend_rec = _published_wmn(N.blend_f64(c.u_cur, u, t), c, fsum)
    st = MN.state_f64(c.xd, o.mean, o.pub_a, c.y, K, fsum)
    o.mu, o.loss = st.mu, st.loss
    o.M = MN.moments_f64(c.xd, o.mean, o.mu, c.y, K, fsum)
    o.H, o.Hd, o.q = wmn_scale_f64(o.M, c.scale, c.n, K, wrong if wrong in SCALE_WRONG else None)
    o.ld = o.H.shape[1]
    if upto == "scale":
        return o
    o.solve = list_solve(o.H, o.q, MN.penalised(K, p), c.u_cur, l2, l1, ridge, fit_intercept, max_sweeps, tol, "mnewton",
                         wrong if wrong in LIST_WRONG else None)
    o.cd_u, o.cd_a, rec = _published_wmn(o.solve.u, c, fsum)
    o.cd_rec = dict(rec, loss=o.loss, sweeps=float(o.solve.sweeps), converged=float(o.solve.converged), negligible=float(o.solve.negligible))
    return o


# ---------------------------------------------------------------------------------------------------------------
# inputs: the smallest that reach each mechanism (the GPU tests and the CPU proof of the bounds use the same ones)
# ---------------------------------------------------------------------------------------------------------------

MIX = dict((name, (l2, l1, ridge)) for name, l2, l1, ridge in PENALTIES)
KINDS = list(N.CANDIDATES)
PENS = list(MIX)

# wnewton, P = p + 1 coordinates (P = 1 does not exist: p >= 1).  What each count sits on:
#   2            the smallest: one slot of wide_column_move, 14 pad rows
#   16, 17       ld = 16 without a pad row; ld = 32 with 15 pad rows (wide_layout.hpp: wide_leading_dim)
#   32, 33       one word of `bits`; the second word (wide_compact: first + 32 < count)
#   64, 65       one wavefront's ballot; the second wavefront (its count in LDS, `before`)
#   256, 257     one compaction step at 256 lanes; the second step, where the count buffers toggle (buf ^= 1)
#   1024, 1025   the same at 1024 lanes; p = 1023 / 1024 are also beyond wide_cd_width's 512: width 0 takes 1024 lanes
# odd and even counts alternate: the last slot of wide_column_move reads the zero pad when the count is odd.
WN_COUNTS = [2, 16, 17, 32, 33, 64, 65, 256, 257, 1024, 1025]
# wmnewton, Q = K (p + 1) (Q >= 4: K >= 2, p >= 1): (K, p).  17 and 257 are prime and no K (p + 1): 18 and 258 stand in
# (ld = 32 with 14 pad rows; the second compaction step at 256 lanes), 15 = 3 x 5 has one pad row.  K = 2 and K = 3 wherever
# the count divides; 65 and 1025 need K = 5.  c % P classifies the intercepts at the block ends (K = 3, p = 1: 1, 3, 5).
WMN_SHAPES = [(2, 1), (3, 1), (3, 4), (2, 7), (3, 5), (2, 15), (3, 10), (2, 31), (5, 12), (3, 21), (3, 84), (2, 127), (3, 85),
              (3, 340), (2, 511), (5, 204), (3, 341)]
WMN_MANY_CLASSES = (20, 12)                   # Q = 260: many classes and few features (210 class pairs)


def wn_case(n, p, centre, sparse_start=False, seed=0):
    """N.dense_case's data at any p (its seed rule); sparse_start: u_cur is 0 but for every seventh coefficient"""
    rng = np.random.default_rng(1000 * n + p + 7919 * seed)
    x = rng.standard_normal((n, p)) * rng.uniform(0.5, 3.0, p) + rng.uniform(-1.0, 1.0, p)
    c = N._finish_case(rng, x, x, np.ones((n, p), dtype=bool), centre, rng.uniform(0.5, 2.0, p))
    if sparse_start:
        c.u_cur = np.where(np.arange(p + 1) % 7 == 3, c.u_cur, 0.0)
        c.u_cur[p] = 0.2
    return c


def wmn_case(n, p, K, centre, sparse_start=False, seed=0):
    c = MN.case(n, p, K, centre, seed=seed)
    if sparse_start:
        b = np.arange(c.Q) % c.P == c.p
        c.u_cur = np.where((np.arange(c.Q) % 7 == 3) | b, c.u_cur, 0.0)
    return c


def constant_column(c):
    """makes the first feature whose coefficient is not 0 in u_cur (in every class) a constant column; returns its index"""
    nz = (np.asarray(c.u_cur).reshape(-1, c.p + 1)[:, :c.p] != 0.0).all(axis=0)
    a = int(np.flatnonzero(nz)[0])
    c.xd[:, a] = 3.0
    c.x = c.xd
    return a


def count_runs(shapes):
    """(shape, centre, kind, penalty): candidates, penalties and centring rotate with the shapes"""
    return [(s, i % 2, KINDS[i % 4], PENS[(i + i // 4) % 3]) for i, s in enumerate(shapes)]


def solve_plan(kind, pen, n, count):
    """MN.converges' rule, less the lasso and the wide candidate with more coordinates than rows (coordinate descent creeps
    there: the float64 restatement does not meet tol = 1e-7 within the 1000 sweeps at 1024 / 1025 coordinates): the cases held
    to convergence and optimality; elsewhere a single list sweep.  tests/test_wide_passes_reference.py shows that the held ones converge."""
    ok = kind in ("zero", "moderate") or (kind == "wide" and pen != "mix1" and 1 < n and count <= n)
    ok = ok and not (pen == "mix1" and count > n)
    return dict(max_sweeps=1000, must_converge=True) if ok else dict(max_sweeps=1)


# The list cases.  Each names its condition; tests/test_wide_passes_reference.py asserts the condition from the restatement.
#   second_screen_adds   a sparse start, lasso: coordinates join after the first list has converged
#   rests_at_zero        a coordinate of the start list ends at an exact 0 and stays listed
#   empty_list           lasso, u_cur = 0, l1 above every |q_j|, the intercept frozen: one sweep, converged, u unchanged
#   exhausted            max_sweeps = 3 at tol = 1e-12: converged = 0
#   single_sweep         max_sweeps = 1 against list_single_sweep_reference
#   frozen_intercept     the intercept(s) bitwise unchanged
def wn_list_case(name):
    c = wn_case(60, 99, 1, sparse_start=True)                # P = 100: the high half of a 64-block, two words beyond
    kw = dict(kind="moderate", l2=0.0, l1=0.02, ridge=False, fit_intercept=True, max_sweeps=1000, tol=1e-7)
    if name == "rests_at_zero":
        kw.update(l1=0.08)
    elif name == "empty_list":
        c.u_cur = np.concatenate([np.zeros(c.p), [0.2]])
        kw.update(l1=10.0, fit_intercept=False)
    elif name == "exhausted":
        kw.update(max_sweeps=3, tol=1e-12)
    elif name == "single_sweep":
        kw.update(max_sweeps=1)
    elif name == "frozen_intercept":
        kw.update(fit_intercept=False, l2=0.01)
    else:
        assert name == "second_screen_adds"
    return c, kw


def wmn_list_case(name):
    c = wmn_case(60, 32, 3, 1, sparse_start=True)            # Q = 99
    kw = dict(kind="moderate", l2=0.0, l1=0.02, ridge=False, fit_intercept=True, max_sweeps=1000, tol=1e-7)
    if name == "rests_at_zero":
        kw.update(l1=0.08)
    elif name == "empty_list":
        b = np.arange(c.Q) % c.P == c.p
        c.u_cur = np.where(b, c.u_cur, 0.0)
        kw.update(l1=10.0, fit_intercept=False)
    elif name == "exhausted":
        kw.update(max_sweeps=3, tol=1e-12)
    elif name == "single_sweep":
        kw.update(max_sweeps=1)
    elif name == "frozen_intercept":
        kw.update(fit_intercept=False, l2=0.01)
    else:
        assert name == "second_screen_adds"
    return c, kw


LIST_CASES = ["second_screen_adds", "rests_at_zero", "empty_list", "exhausted", "single_sweep", "frozen_intercept"]


# The limits: p = 5819 (wnewton) and K = 2, p = 2909 (wmnewton), Q = P = 5820, at n = 40, a sparse start and penalties under
# which the float64 restatement converges well within the 1000 sweeps (tests/test_wide_passes_reference.py asserts it).
LIMIT_PENALTY = dict(l2=0.2, l1=0.4, ridge=False)
WMN_LIMIT_PENALTY = dict(l2=0.5, l1=0.4, ridge=False)


def wn_limit_case():
    return wn_case(40, WNEWTON_MAX_FEATURES, 1, sparse_start=True)


def wmn_limit_case():
    return wmn_case(40, WMNEWTON_MAX_COORDINATES // 2 - 1, 2, 1, sparse_start=True)

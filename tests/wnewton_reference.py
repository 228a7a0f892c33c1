"""sa.sgdnet_wnewton (SGDNET_MODE_WNEWTON, sgdnet_amd/csrc/newton.hip: wide_scale_kernel and newton_wide_cd_kernel)
restated in numpy, and the inputs its tests share: tests/test_gpu_wnewton.py runs them on the device,
tests/test_wnewton_host.py runs the restatement on the same inputs on the CPU.

The outer loop is tests/test_gpu_newton.py::numpy_newton_path's (state, weighted moments, inner solve, accept / halve, the
stopping rule).  The inner solve, about the iterate u_cur:
  start    u = u_cur, so g = H (u - u_cur) - q = -q exactly; the list is {j < p : u_j != 0} and the intercept coordinate
           when it is fitted (unpenalised, without threshold; frozen: never visited)
  screen   every j < p outside the list gets the coordinate update from u_j = 0; those that would move join the list,
           which stays in ascending order of j
  sweep    newton mode's coordinate update over the list; a move by d does g += H[:, j] d for ALL k, so g stays the full
           gradient.  The sweeps end as newton mode's do (max|du| / max|u| <= tol, all zero, or negligible); then the
           screen runs again, and the solve is done when a screen adds nothing.
MAX_SWEEPS bounds the list sweeps of one solve; a solve cut short is continued by the next outer step."""
import numpy as np
import scipy.sparse as sp

import test_gpu_newton as tn

THRESH = 1e-12                            # what every GPU fit of the tests passes
LDS_BYTES = 160 * 1024
ALL_SETTINGS = [(True, True), (True, False), (False, True), (False, False)]      # (intercept, standardize)
DEFAULTS = [(True, True)]
MAX_HALVINGS, OBJECTIVE_SLACK, MAX_SWEEPS, NEGLIGIBLE = tn.MAX_HALVINGS, tn.OBJECTIVE_SLACK, tn.MAX_SWEEPS, tn.NEGLIGIBLE


def state_bytes(P):
    """newton.hpp: g, u and diag H (3 P doubles), P list words, one bit per coordinate in whole words, the compaction's
    2 x 16 counts; P = p + 1"""
    return 24 * P + 4 * P + 4 * ((P + 31) // 32) + 4 * 2 * 16


def derived_limit():
    """the largest p whose P = p + 1 coordinates fit one workgroup's LDS"""
    p = 1
    while state_bytes(p + 2) <= LDS_BYTES:
        p += 1
    return p


LIMIT = derived_limit()                   # sgdnet_wnewton_max_features(): 5819


def numpy_wide_newton_path(x, y, lam, mix, standardize=True, intercept=True, thresh=THRESH, maxit=1000):
    """(a0 (L,), beta (p, L), info); info: steps and codes per lambda, passes and halvings of the path, per lambda the most
    screens and list sweeps of one inner solve."""
    x = np.asarray(x.todense()) if sp.issparse(x) else np.asarray(x, dtype=float)
    n, p = x.shape
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    sd = np.where(var == 0, 1.0, np.sqrt(var)) if standardize else np.ones(p)
    m = mean if (standardize or intercept) else np.zeros(p)
    centre = mean if standardize else np.zeros(p)                 # the driver's x_center
    Z = np.column_stack([(x - m) / sd, np.ones(n)])
    ybar = min(max(y.mean(), 1e-9), 1 - 1e-9)
    u = np.zeros(p + 1)
    u[p] = np.log(ybar / (1 - ybar)) if intercept else 0.0
    ridge = mix == 0

    def state(u):
        eta = Z @ u
        e = np.exp(eta)
        t = 1.0 / (1.0 + e)
        return t * (1 - t), t - (1 - y), (np.log(1 + e) - y * eta).mean()

    def penalty(u, l1, l2):
        return l2 * 0.5 * (u[:p] ** 2).sum() + l1 * np.abs(u[:p]).sum()

    v, r, loss = state(u)
    info = dict(halvings=0, steps=[], codes=[], passes=1, screens=[], sweeps=[])
    a0, beta = [], []
    for l in lam:
        l1, l2 = (0.0 if ridge else mix * l), (1 - mix) * l
        objective = loss + penalty(u, l1, l2)
        steps, converged, most_screens, most_sweeps = 0, False, 0, 0
        while steps < maxit and not converged:
            H, q = (Z * v[:, None]).T @ Z / n, Z.T @ r / n
            diag = np.diag(H).copy()
            c, g = u.copy(), -q.copy()
            in_list = np.append(c[:p] != 0.0, bool(intercept))
            inner = negligible = False
            sweeps = screens = 0
            while True:
                # the screen: the coordinate update from u_j = 0 for every feature at once
                z, den = -g[:p], diag[:p] + l2
                nu0 = z if ridge else np.where(z > l1, z - l1, np.where(z < -l1, z + l1, 0.0))
                with np.errstate(divide="ignore", invalid="ignore"):
                    nu0 = np.where(den > 0, nu0 / den, 0.0)
                added = (nu0 != 0.0) & ~in_list[:p]
                screens += 1
                if screens > 1 and not added.any():
                    inner = True
                    break
                in_list[:p] |= added
                live = np.flatnonzero(in_list)
                met = False
                while sweeps < MAX_SWEEPS and not met:
                    change = size = eta_sq = 0.0
                    for j in live:
                        z, den = H[j, j] * c[j] - g[j], H[j, j] + (l2 if j < p else 0.0)
                        nu = z
                        if j < p and not ridge:
                            nu = z - l1 if z > l1 else (z + l1 if z < -l1 else 0.0)
                        nu = nu / den if den > 0 else (0.0 if j < p else c[j])
                        d = nu - c[j]
                        change, size, eta_sq = max(change, abs(d)), max(size, abs(nu)), max(eta_sq, nu * nu * H[j, j])
                        if d != 0.0:
                            c[j] = nu
                            g += H[j] * d                                   # (H is symmetric: row j is column j)
                    sweeps += 1
                    negligible = eta_sq <= NEGLIGIBLE ** 2                  # zero to rounding (newton.hpp)
                    met = (size == 0 and change == 0) or (size != 0 and change / size <= thresh) or negligible
                if not met:
                    break
            most_screens, most_sweeps = max(most_screens, screens), max(most_sweeps, sweeps)
            v, r, cl = state(c)
            info["passes"] += 1
            candidate = cl + penalty(c, l1, l2)
            h = 0
            while h < MAX_HALVINGS and np.abs(c - u).max() > 0 and not candidate <= objective + OBJECTIVE_SLACK * abs(objective):
                c = u + 0.5 * (c - u)
                v, r, cl = state(c)
                info["passes"] += 1
                candidate = cl + penalty(c, l1, l2)
                h += 1
                negligible = False
            info["halvings"] += h
            change, size = np.abs(c - u).max(), np.abs(c).max()
            u, loss, objective = c, cl, candidate
            steps += 1
            converged = inner and ((size == 0 and change == 0) or (size != 0 and change / size <= thresh) or negligible)
        info["steps"].append(steps)
        info["codes"].append(0 if converged else 1)
        info["screens"].append(most_screens)
        info["sweeps"].append(most_sweeps)
        b = u[:p] / sd
        beta.append(b)
        a0.append(u[p] - (m - centre) @ b - centre @ b if intercept else 0.0)
    return np.array(a0), np.array(beta).T, info


automatic_lambdas = tn.automatic_lambdas


# ---- the inputs ----
# (n, p); p = None: the feature limit.  (40, 1): two coordinates; (63, 14) and (65, 15): p + 2 on both sides of a 16-column
# tile; (300, 199): the first p mode = newton refuses; (65, 255) and (65, 256): P = p + 1 on both sides of one stride of
# the 256-lane workgroup and of a bit word; (65, 1024): P one past a stride of the 1024-lane one; (40, limit): the whole
# LDS budget.
SHAPES = [(40, 1), (63, 14), (65, 15), (300, 199), (65, 255), (65, 256), (65, 1024), (40, None)]
MIXES = [0.0, 0.5, 1.0]
BOTH_MODES = [(600, 198), (200, 33)]      # where mode = newton runs too
# Further dense inputs of the width test, where the list compaction (csrc/wide_cd_device.hpp) can go wrong over the
# P = p + 1 coordinates: a single feature; a bit word without and with its upper half (P = 31, 33); a wavefront boundary
# (P = 64, 65); one stride of the 256-lane workgroup from both sides (P = 255, 256, 257); odd and even slot tails
WIDTH_SHAPES = [(65, p) for p in (1, 30, 32, 63, 64, 254, 255, 256)]
BOTH_MODES_PATH = dict(nlambda=6, lambda_min_ratio=1e-2)


def path_of(n, p, mix):
    """(nlambda, lambda_min_ratio) of the automatic path a shape is fitted with.  At p > n the classes separate: the
    unpenalised end of the path does not exist, and the ratio keeps away from it."""
    if p is None:
        return (2, 0.3) if mix == 0.0 else (3, 0.2)      # (ridge: every sweep moves all 5820 coordinates)
    if p >= 255:
        return (4, 1e-2) if mix == 0.0 else (4, 0.1)
    return (6, 1e-2)


def settings_of(p):
    return ALL_SETTINGS if p is not None and p <= 256 else DEFAULTS


def large_mean_twins(sparse):
    """tests/test_gpu_newton.py::test_large_mean_column_does_not_cancel's input: (shifted, centred, y), the same matrix with
    one column of sd 1 at mean 1e6 (every entry stored) and at mean 0; the column carries most of the signal."""
    x, _ = tn.problem(200, 5, sparse, seed=7)
    rng = np.random.default_rng(11)
    col = rng.standard_normal(200)
    col = (col - col.mean()) / col.std()
    xd = np.asarray(x.todense()) if sparse else x.copy()
    shifted, centred = xd.copy(), xd.copy()
    shifted[:, 2], centred[:, 2] = 1e6 + col, col
    eta = 0.4 * (centred[:, 0] - centred[:, 0].mean()) + 1.2 * col
    y = (rng.random(200) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    wrap = sp.csc_matrix if sparse else np.asarray
    return wrap(shifted), wrap(centred), y


LARGE_MEAN = dict(alpha=0.5, nlambda=10, lambda_min_ratio=0.05)
LARGE_MEAN_TOL = tn.ORACLE_TOL            # the bound newton mode meets on this input (tests/test_gpu_newton.py)


def rescreen_problem():
    """An input on which, inside one inner solve, the list converges and a later screen still adds to it: strongly
    correlated columns (three factors behind 300 features), six of them carrying the log-odds.
    test_wnewton_host.py asserts the screens."""
    rng = np.random.default_rng(1)
    n, p = 80, 300
    f, A = rng.standard_normal((n, 3)), rng.standard_normal((3, p))
    x = f @ A + 0.8 * rng.standard_normal((n, p))
    B = np.zeros(p)
    B[:6] = [3, -3, 2, -2, 1.5, -1.5]
    eta = (x @ B) / 4.0
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    return x, y


RESCREEN = dict(alpha=0.5, nlambda=3, lambda_min_ratio=0.1)

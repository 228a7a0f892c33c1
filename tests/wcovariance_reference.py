"""sa.sgdnet_wcovariance (SGDNET_MODE_WCOVARIANCE, sgdnet_amd/csrc/covariance.hip: cov_wide_path_kernel) restated in numpy,
and the inputs its tests share: tests/test_gpu_wcovariance.py runs them on the device, tests/test_wcovariance_host.py
runs the restatement on the same inputs on the CPU.

The algorithm, per lambda and warm-started from the one before:
  rebuild  the list becomes {j : w_j != 0}; g = sum_{j in list} S[:, j] w_j - c~ afresh
  screen   every j outside the list gets the coordinate update from w_j = 0; those that would move join the list, which
           stays in ascending order of j
  sweep    cyclic coordinate descent over the list; a move by d does g += S[:, j] d for ALL k, so g stays the full
           gradient.  A sweep ends with the reference's ConvergenceCheck over the list (max|dw| / max|w| <= tol, all
           zero counts as converged); when it is met the screen runs again, and the lambda is done when a screen adds
           nothing.
max_sweeps bounds the list sweeps of one lambda.  Units as in tests/test_gpu_covariance.py::numpy_cd_path."""
import numpy as np
import scipy.sparse as sp

import test_gpu_covariance as tc

THRESH, MAXIT = 1e-12, 1_000_000          # what every GPU fit of the tests passes
LIMIT = 4531                              # sgdnet_wcovariance_max_features(): test_wcovariance_host.py derives it
ALL_SETTINGS = [(True, True), (True, False), (False, True), (False, False)]      # (intercept, standardize)
DEFAULTS = [(True, True)]


def new_w(sjj, wj, gj, l2, l1, ridge):
    z, den = sjj * wj - gj, sjj + l2
    nw = z if ridge else (z - l1 if z > l1 else (z + l1 if z < -l1 else 0.0))
    return nw / den if den > 0 else 0.0


def numpy_wide_path(x, y, lam, mix, standardize=True, intercept=True, tol=THRESH, max_sweeps=MAXIT):
    """(a0, beta (p, L), sweeps (L), screens (L), unconverged (L))"""
    x = np.asarray(x.todense()) if sp.issparse(x) else np.asarray(x, dtype=float)
    n, p = x.shape
    ym, ys = y.mean(), (y.std() if y.std() != 0 else 1.0)
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    sd = np.where(var == 0, 1.0, np.sqrt(var)) if standardize else np.ones(p)
    mu = mean if (standardize or intercept) else np.zeros(p)
    xt, yt = (x - mu) / sd, (y - ym) / ys
    S, c = xt.T @ xt / n, xt.T @ yt / n
    diag = np.diag(S).copy()
    ridge = mix == 0
    w = np.zeros(p)
    a0, beta, n_sweeps, n_screens, unconverged = [], [], [], [], []
    for l in lam:
        l1, l2 = mix * l / ys, (1 - mix) * l / ys
        in_list = w != 0.0
        live = np.flatnonzero(in_list)
        g = S[:, live] @ w[live] - c
        sweeps, screens, converged = 0, 0, False
        while True:
            # the screen: new_w from w_j = 0 for every j at once; a coordinate outside the list joins when it is not 0
            z = -g
            nw0 = z if ridge else np.where(z > l1, z - l1, np.where(z < -l1, z + l1, 0.0))
            with np.errstate(divide="ignore", invalid="ignore"):
                nw0 = np.where(diag + l2 > 0, nw0 / (diag + l2), 0.0)
            added = (nw0 != 0.0) & ~in_list
            screens += 1
            if screens > 1 and not added.any():
                converged = True
                break
            in_list |= added
            live = np.flatnonzero(in_list)
            met = False
            while sweeps < max_sweeps and not met:
                change = size = 0.0
                for j in live:
                    nw = new_w(diag[j], w[j], g[j], l2, l1, ridge)
                    d = nw - w[j]
                    change, size = max(change, abs(d)), max(size, abs(nw))
                    if d != 0.0:
                        w[j] = nw
                        g += S[:, j] * d
                sweeps += 1
                met = (size == 0.0 and change == 0.0) or (size != 0.0 and change / size <= tol)
            if not met:
                break
        beta.append(w * ys / sd)
        a0.append(ym - mean @ beta[-1] if intercept else 0.0)
        n_sweeps.append(sweeps)
        n_screens.append(screens)
        unconverged.append(not converged)
    return np.array(a0), np.array(beta).T, np.array(n_sweeps), np.array(n_screens), np.array(unconverged)


def automatic_lambdas(x, y, mix, standardize, nlambda, ratio):
    """regularization_path / lambda_max of the driver for a gaussian response (driver.cpp), as tests/test_covariance_host.py"""
    import sgdnet_amd as sa
    xd = np.asarray(x.todense()) if sp.issparse(x) else x
    xc, xs = sa.feature_moments(x, standardize)
    lmax = np.abs(((xd - xc) / xs).T @ (y - y.mean())).max() / len(y) / max(mix, 0.001)
    return np.exp(np.linspace(np.log(lmax), np.log(lmax * ratio), nlambda))


# ---- the inputs ----
# (n, p); p = None: the feature limit.  (2, 1): one coordinate; (63, 15): one tile, one stride; (300, 199): the first p
# mode = covariance refuses, p odd (the last 16-byte slot is half pad); (65, 257): one past a stride of the 256-lane
# workgroup; (65, 1025): one past a stride of the 1024-lane one; (40, limit): the whole LDS budget.
SHAPES = [(2, 1), (63, 15), (300, 199), (65, 257), (65, 1025), (40, None)]
MIXES = [0.0, 0.5, 1.0]
# Further dense inputs of the width test, where the list compaction (csrc/wide_cd_device.hpp) can go wrong: a single
# coordinate; a bit word without and with its upper half (31, 33); a wavefront boundary (64, 65); one stride of the
# 256-lane workgroup from both sides (255, 256, 257); odd and even slot tails; the first p of the look-ahead instance (1537)
WIDTH_SHAPES = [(65, p) for p in (1, 31, 33, 64, 65, 255, 256, 257, 1537)]
WIDTH_PATH = dict(nlambda=5, lambda_min_ratio=5e-2)       # (the feature limit has its own in the test)


def path_of(n, p, mix):
    """(nlambda, lambda_min_ratio) of the automatic path a shape is fitted with"""
    if p is None:
        return (3, 0.1) if mix == 0.0 else (4, 0.1)
    if p in (257, 1025):                 # p > n: the lasso end of a long path takes 10^4 sweeps and more
        return (4, 1e-2) if mix == 0.0 else (5, 5e-2)
    return (6, 1e-2)


def settings_of(p):
    return ALL_SETTINGS if p is not None and p <= 257 else DEFAULTS


def large_mean_problem(sparse):
    """tests/test_gpu_covariance.py's problem() at (63, 15) with one column of mean 1e6 and sd 1 (every entry stored)"""
    x, y = tc.problem(63, 15, sparse, seed=7)
    col = np.random.default_rng(11).standard_normal(63)
    col = (col - col.mean()) / col.std()
    xd = np.asarray(x.todense()) if sparse else x.copy()
    xd[:, 2] = 1e6 + col
    return (sp.csc_matrix(xd) if sparse else xd), y + 0.7 * col


def rescreen_problem():
    """An input on which the list converges and a later screen still adds to it: strongly correlated columns (three
    factors behind 300 features), six of them carrying the response.  test_wcovariance_host.py asserts the screens."""
    rng = np.random.default_rng(1)
    n, p = 50, 300
    f, A = rng.standard_normal((n, 3)), rng.standard_normal((3, p))
    x = f @ A + 0.3 * rng.standard_normal((n, p))
    B = np.zeros(p)
    B[:6] = [3, -3, 2, -2, 1.5, -1.5]
    y = x @ B + 0.1 * rng.standard_normal(n)
    return x, y


RESCREEN = dict(alpha=0.5, nlambda=3, lambda_min_ratio=1e-2)

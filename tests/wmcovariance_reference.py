"""sa.sgdnet_wmcovariance (SGDNET_MODE_WMCOVARIANCE, sgdnet_amd/csrc/covariance.hip: cov_wide_group_path_kernel) restated in
numpy, and the inputs its tests share: tests/test_gpu_wmcovariance.py runs them on the device,
tests/test_wmcovariance_host.py runs the restatement on the same inputs on the CPU.

The algorithm, per lambda and warm-started from the one before, a block the K coefficients w_j. of a feature:
  rebuild  the list becomes {j : w_j. != 0}; g = sum_{j in list} S[:, j] w_j. - c~ afresh (p x K)
  screen   every j outside the list gets the block update from w_j. = 0; the blocks that would move join the list, which
           stays in ascending order of j
  sweep    cyclic block coordinate descent over the list; a move by d (K) does g += S[:, j] d' for ALL k, so g stays
           the full gradient.  A sweep ends with the reference's ConvergenceCheck over the list (max|dw| / max|w| <= tol,
           all zero counts as converged); when it is met the screen runs again, and the lambda is done when a screen adds
           nothing.
max_sweeps bounds the list sweeps of one lambda.  Units, preprocessing and the block update as in
tests/test_gpu_mcovariance.py::numpy_block_cd_path, which sweeps over all p blocks instead."""
import numpy as np
import scipy.sparse as sp

import test_gpu_mcovariance as tm
from test_gpu_mcovariance import DEV_TOL, KKT_BOUND, numpy_block_cd_path, numpy_kkt, problem  # noqa: F401

THRESH, MAXIT = 1e-12, 1_000_000          # what every GPU fit of the tests passes
# sgdnet_wmcovariance_max_features(K): test_wmcovariance_host.py derives them from the budget written in covariance.hpp
LIMITS = {1: 4531, 2: 3709, 3: 2722, 10: 950, 96: 104}
LDS_BYTES = 160 * 1024
MAX_COLUMNS = 4531 + 1                    # p + K of the moments pass: sgdnet_wcovariance_max_features() + 1

# The distance of two stopped iterations from each other.  Over every input of inputs() below (test_wmcovariance_host.py::
# test_restatement_agrees_with_the_full_sweeps measures them and asserts these pins): the largest difference of the
# restatement's coefficients and intercepts from numpy_block_cd_path's relative to max|beta| of the path, and the largest difference of
# their dev_ratio.  The device's comparison against sa.sgdnet_mcovariance allows 10 x these (both sides stop at thresh: the
# project's convention for a measured distance, test_gpu_mcovariance.py: ORACLE_REL_CHANGE).
BLOCK_CD_REL = 6.0e-11                    # measured 5.32e-11 (intercepts; coefficients 3.59e-11, the re-screen input)
BLOCK_CD_DEV = 1.3e-13                    # measured 1.13e-13


def state_bytes(p, K):
    """g and w: 2 K vectors of p rounded up to even doubles; diag S; K doubles of scratch; p list words, one bit per
    block in whole words, the compaction's 2 x 16 counts"""
    return 16 * K * (p + (p & 1)) + 8 * p + 8 * K + 4 * p + 4 * ((p + 31) // 32) + 4 * 2 * 16


def fits(p, K):
    return state_bytes(p, K) <= LDS_BYTES and p + K <= MAX_COLUMNS


def max_features(K):
    if K < 1 or not fits(1, K):
        return 0
    p = 1
    while fits(p + 1, K):
        p += 1
    return p


def block_new_w(sjj, wj, gj, l2, l1, ridge):
    """group_new_w over a block: shrink * (S_jj w_j. - g_j.) / (S_jj + l2)"""
    z, den = sjj * wj - gj, sjj + l2
    nz = np.sqrt((z * z).sum())
    if not nz > 0.0 or not den > 0.0:
        return np.zeros_like(wj)
    shrink = 1.0 if ridge else (1.0 - l1 / nz if nz > l1 else 0.0)
    return shrink * z / den


def numpy_wide_group_path(x, y, lam, mix, standardize=True, intercept=True, standardize_response=False, tol=THRESH, max_sweeps=MAXIT):
    """(a0 (K, L), beta (K, p, L), dev_ratio (L), sweeps (L), screens (L), added (L lists: the blocks each screen added),
    unconverged (L))"""
    x, y = tm.dense(x), tm.preprocessed_response(y, standardize_response)
    n, p = x.shape
    K = y.shape[1]
    b0 = y.mean(axis=0)
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    sd = np.where(var == 0, 1.0, np.sqrt(var)) if standardize else np.ones(p)
    mu = mean if (standardize or intercept) else np.zeros(p)
    xt, yt = (x - mu) / sd, y - b0
    S, c = xt.T @ xt / n, xt.T @ yt / n
    diag = np.diag(S).copy()
    yy, nulldev = (yt ** 2).sum(), ((y - y.mean(axis=0)) ** 2).sum()
    ridge = mix == 0
    w = np.zeros((p, K))
    a0, beta, dev_ratio, n_sweeps, n_screens, all_added, unconverged = [], [], [], [], [], [], []
    for l in lam:
        l1, l2 = mix * l, (1 - mix) * l
        in_list = (w != 0.0).any(axis=1)
        live = np.flatnonzero(in_list)
        g = S[:, live] @ w[live] - c
        sweeps, screens, converged, added_by = 0, 0, False, []
        while True:
            # the screen: the block update from w_j. = 0 for every j at once; a block outside the list joins when it moves
            nz = np.sqrt((g * g).sum(axis=1))
            den = diag + l2
            with np.errstate(divide="ignore", invalid="ignore"):
                shrink = np.ones(p) if ridge else np.where(nz > l1, 1.0 - l1 / nz, 0.0)
                shrink = np.where((nz > 0.0) & (den > 0.0), shrink, 0.0)
                nw0 = shrink[:, None] * -g / np.where(den > 0.0, den, 1.0)[:, None]
            added = (nw0 != 0.0).any(axis=1) & ~in_list
            screens += 1
            added_by.append(int(added.sum()))
            if screens > 1 and not added.any():
                converged = True
                break
            in_list |= added
            live = np.flatnonzero(in_list)
            met = False
            while sweeps < max_sweeps and not met:
                change = size = 0.0
                for j in live:
                    nw = block_new_w(diag[j], w[j], g[j], l2, l1, ridge)
                    d = nw - w[j]
                    change, size = max(change, np.abs(d).max()), max(size, np.abs(nw).max())
                    if d.any():
                        w[j] = nw
                        g += np.outer(S[:, j], d)
                sweeps += 1
                met = (size == 0.0 and change == 0.0) or (size != 0.0 and change / size <= tol)
            if not met:
                break
        b = w / sd[:, None]
        beta.append(b.T.copy())
        a0.append(b0 - mean @ b if intercept else b0.copy())
        dev_ratio.append(1.0 - (yy - n * (w * (c - g)).sum()) / nulldev if nulldev > 0 else 0.0)
        n_sweeps.append(sweeps)
        n_screens.append(screens)
        all_added.append(added_by)
        unconverged.append(not converged)
    return (np.array(a0).T, np.moveaxis(np.array(beta), 0, 2), np.array(dev_ratio), np.array(n_sweeps), np.array(n_screens), all_added,
            np.array(unconverged))


def automatic_lambdas(x, y, mix, standardize, nlambda, ratio, standardize_response=False):
    """regularization_path / lambda_max of the driver for an mgaussian response (driver.cpp): the largest row norm of
    X~'(Y - mean) / n over max(mix, 0.001), then nlambda values down to ratio of it on a log scale"""
    import sgdnet_amd as sa
    xd, yd = tm.dense(x), tm.preprocessed_response(y, standardize_response)
    xc, xs = sa.feature_moments(x, standardize)
    c = ((xd - xc) / xs).T @ (yd - yd.mean(axis=0)) / len(yd)
    lmax = np.sqrt((c * c).sum(axis=1)).max() / max(mix, 0.001)
    return np.exp(np.linspace(np.log(lmax), np.log(lmax * ratio), nlambda))


# ---- the inputs ----
# (n, p, K) at the kernel's edges.  (5, 1, 2): one block; (37, 2, 3): one slot; (63, 15 / 16 / 17, 4): around the leading
# dimension of S (16), p odd and even; (65, 13, 5): the responses cross a 16-column tile edge of the moments pass;
# (80, 65, 2): one past a wavefront of the list compaction; (120, 513, 2): p odd, one slot beyond a stride of 256 lanes;
# (90, 1025, 3): one slot beyond a stride of 1024 lanes and the first p the 1024-lane workgroup takes by the rule.
SHAPES = [(5, 1, 2), (37, 2, 3), (63, 15, 4), (63, 16, 4), (63, 17, 4), (65, 13, 5), (80, 65, 2), (120, 513, 2), (90, 1025, 3)]
LIMIT_SHAPES = [(40, None, 2), (40, None, 10)]                 # p = None: wmcovariance_max_features(K)
LIMIT_PATH = dict(nlambda=4, lambda_min_ratio=0.1)
MIXES = [1.0, 0.5, 0.0]
ALL_SETTINGS = [(True, True), (True, False), (False, True), (False, False)]      # (intercept, standardize)
DEFAULTS = [(True, True)]
BOTH_MODES = [(300, 195, 2), (300, 174, 10), (200, 33, 3)]     # where sa.sgdnet_mcovariance runs too (the first two at its limit)
BOTH_PATH = dict(nlambda=6, lambda_min_ratio=1e-2)
WIDTH_SHAPES = [((90, 1025, 3), False), ((90, 1025, 3), True), ((63, 15, 4), False), ((40, None, 2), False)]
NONMONOTONE_SHAPE = (300, 199, 2)


def path_of(p, mix):
    """(nlambda, lambda_min_ratio) of the automatic path a shape is fitted with: 6 lambdas; p > n stops at a tenth of
    lambda_max (the lasso end of a longer path takes 10^3 sweeps and more, minutes of the numpy restatement)"""
    return (6, 0.1) if p >= 513 else (6, 1e-2)


def settings_of(p):
    return ALL_SETTINGS if p <= 65 else DEFAULTS


def large_mean_problem(sparse):
    """problem() at (63, 15, 4) with one column of mean 1e6 and sd 1 (every entry stored) that all responses load on"""
    x, y = problem(63, 15, 4, sparse, seed=7)
    col = np.random.default_rng(11).standard_normal(63)
    col = (col - col.mean()) / col.std()
    xd = tm.dense(x).copy()
    xd[:, 2] = 1e6 + col
    return (sp.csc_matrix(xd) if sparse else xd), y + np.outer(col, [0.7, -0.4, 0.2, 0.5])


def rescreen_problem():
    """K = 2 analogue of wcovariance_reference.rescreen_problem: strongly correlated columns (three factors behind 80
    features), six of them carrying the two responses: at the last lambda the list converges and a later screen still
    adds a block.  test_wmcovariance_host.py asserts the screens."""
    rng = np.random.default_rng(3)
    n, p = 50, 80
    f, A = rng.standard_normal((n, 3)), rng.standard_normal((3, p))
    x = f @ A + 0.3 * rng.standard_normal((n, p))
    B = np.zeros((p, 2))
    B[:6, 0] = [3, -3, 2, -2, 1.5, -1.5]
    B[:6, 1] = [-1, 2, 2, -3, 0.5, 1.5]
    y = x @ B + 0.1 * rng.standard_normal((n, 2))
    return x, y


RESCREEN = dict(alpha=0.5, nlambda=6, lambda_min_ratio=1e-2)


def inputs():
    """Every (what, x, y, lambdas, mix, standardize, intercept, standardize_response) the device fits outside the limit
    shapes and the refusals: what test_wmcovariance_host.py runs the restatement on"""
    for n, p, K in SHAPES:
        for sparse in (False, True):
            x, y = problem(n, p, K, sparse)
            for mix in MIXES:
                for intercept, standardize in settings_of(p):
                    lam = automatic_lambdas(x, y, mix, standardize, *path_of(p, mix))
                    yield ("shape", n, p, K, sparse, mix, intercept, standardize), x, y, lam, mix, standardize, intercept, False
    for sparse in (False, True):
        x, y = problem(65, 13, 5, sparse, seed=1)
        yield ("standardize_response", sparse), x, y, automatic_lambdas(x, y, 0.5, True, 6, 1e-2, True), 0.5, True, True, True
        x, y = large_mean_problem(sparse)
        yield ("mean 1e6", sparse), x, y, automatic_lambdas(x, y, 0.5, True, 6, 1e-2), 0.5, True, True, False
        for n, p, K in BOTH_MODES:
            x, y = problem(n, p, K, sparse, seed=3)
            for mix in (0.5, 0.0):
                lam = automatic_lambdas(x, y, mix, True, BOTH_PATH["nlambda"], BOTH_PATH["lambda_min_ratio"])
                yield ("both modes", n, p, K, sparse, mix), x, y, lam, mix, True, True, False
        x, y = problem(*NONMONOTONE_SHAPE, sparse, seed=1)
        yield ("user lambdas", sparse), x, y, np.array(tm.NONMONOTONE), 0.5, True, True, False
    x, y = rescreen_problem()
    lam = automatic_lambdas(x, y, RESCREEN["alpha"], True, RESCREEN["nlambda"], RESCREEN["lambda_min_ratio"])
    yield ("re-screen",), x, y, lam, RESCREEN["alpha"], True, True, False

"""Cross-validation in wide multi-response covariance mode (sa.cv_wmcovariance_fits -> sgdnet_cv_wmcovariance_*,
sgdnet_amd/csrc/covariance.hip: wmcovariance_cv_run): the inputs and the numpy its tests share.
tests/test_gpu_cv_wmcovariance.py runs them on the device, tests/test_cv_wmcovariance_host.py checks on the CPU what needs no
device.  Inputs and numpy only: nothing here touches a GPU.

Tolerances (the project's own; none is derived from what the code under test returns)
  KKT_BOUND      1e-8   KKT ratio <= 1e-8, intercept residual <= 1e-8 * lambda (tests/test_gpu_mcovariance.py: assert_optimal)
  SAME_OPTIMUM   1e-9   "the same optimum reached twice", with the a0 rule and the df / dfmat equality of
                        tests/test_gpu_cv_mcovariance.py: assert_same_fit
  POOLING_BOUND  1e-12  pooled against direct moments (tests/test_cv_mcovariance_host.py)"""
import numpy as np
import scipy.sparse as sp

import cv_wcovariance_reference as cw
import test_gpu_cv_mcovariance as tcm
import wmcovariance_reference as wm
from cv_wcovariance_reference import equal_folds, leading_dim, rows_per_chunk, sorted_folds, tile_pairs, training_sets, unequal_folds  # noqa: F401

KKT_BOUND = wm.KKT_BOUND
SAME_OPTIMUM = tcm.SAME_OPTIMUM
POOLING_BOUND = 1e-12
TIGHT = dict(thresh=wm.THRESH, maxit=wm.MAXIT)
LIMITS = wm.LIMITS
MIXES = [0.0, 0.5, 1.0]
assert KKT_BOUND == 1e-8 and SAME_OPTIMUM == 1e-9 and TIGHT == dict(thresh=1e-12, maxit=1_000_000)

# (n, p, K, G)
#   (12, 1, 2, 2)       one block
#   (195, 13, 5, 3)     groups of 65 rows, one past the 64-row stage; the responses cross the 16-column tile edge
#   (192, 14, 2, 3)     groups of exactly 64 rows; Pa = 17: the ones column alone in the second tile
#   (189, 15 / 16 / 17, 4, 3)   around ld = 16: p odd and even (the pad slot); the set stride ld p != p^2
#   (600, 196, 2, 3)    the first p the narrow CV refuses at K = 2
#   (130, 513, 2, 2)    one slot past a 256-lane stride, p > n_T
#   (130, 1025, 3, 2)   the 1024-lane kernel, chosen by the width rule (one mix per case)
SHAPES = [(12, 1, 2, 2), (195, 13, 5, 3), (192, 14, 2, 3), (189, 15, 4, 3), (189, 16, 4, 3), (189, 17, 4, 3), (600, 196, 2, 3),
          (130, 513, 2, 2), (130, 1025, 3, 2)]
SMALL_SHAPES = [s for s in SHAPES if s[1] <= 17]      # what the CPU restatements run on
LIMIT_SHAPES = [(80, 2, 2), (80, 10, 2)]             # (n, K, G): p = LIMITS[K]; dense only, mix 0.5
LIMIT_PATH = (4, 0.1)
NARROW_SHAPES = [(195, 13, 5, 3), (600, 195, 2, 3)]   # where sa.cv_mcovariance_fits runs too (the second at its limit)
FIRST_REFUSED = (600, 196, 2, 3)
MANY_JOBS = (90, 3, 2, 90)       # leave-one-out, "rest", three mixes: 270 jobs on 256 compute units
LARGE_MEAN_PATH = dict(nlambda=10, lambda_min_ratio=0.05)

# The byte budget of wmcovariance_cv_run (csrc/covariance.hpp: kWcovCvBytes, wmcov_cv_bytes); test_cv_wmcovariance_host.py
# holds this copy against the constant the library reports in its refusal.
BUDGET_BYTES = 16 << 30


def row_chunks(n, p, K, counts):
    """the dense group moments pass cuts its chunks at the groups' ends (csrc/covariance.hip: wmcov_cv_row_chunks)"""
    r = rows_per_chunk(n, p + K + 1)
    return int(sum((c + r - 1) // r for c in counts))


def budget_bytes(G, p, K, chunks):
    """group moments + their total + the dense partial tiles + the scaled matrices + c~, in bytes (chunks = 0: sparse x)"""
    Pa = p + K + 1
    return 8 * ((G + 1) * Pa ** 2 + chunks * tile_pairs(Pa) * 256 + G * leading_dim(p) * p + G * p * K)


def groups_over_budget(p, K):
    """the fewest groups of one row each whose dense CV at p features and K responses is over the budget"""
    G = 1
    while budget_bytes(G, p, K, G) <= BUDGET_BYTES:
        G += 1
    return G


def path_of(n, p, G):
    """(nlambda, lambda_min_ratio): 6 lambdas down to 1e-2 lambda_max; down to 0.1 lambda_max where p is above the smallest
    training set (a fold of "fold" mode: n // G rows)"""
    return (6, 0.1) if p > n // G else (6, 1e-2)


def problem(n, p, K, sparse, seed=0):
    """tests/test_gpu_cv_mcovariance.py: problem"""
    return tcm.problem(n, p, K, sparse, seed)


def large_mean_problem(n, p, K, sparse):
    """problem() with column 2 of mean 1e6 and sd 1 (every entry stored) that every response loads on: the input of
    tests/test_gpu_cv_mcovariance.py: test_large_mean_column"""
    x, y = problem(n, p, K, sparse, seed=6)
    xd = np.asarray(x.todense()) if sparse else x.copy()
    col = np.random.default_rng(11).standard_normal(n)
    xd[:, 2] = 1e6 + (col - col.mean()) / col.std()
    return (sp.csr_matrix(xd) if sparse else xd), y + 0.7 * col[:, None]


def lambdas(x, y, mix, standardize, nlambda, ratio, standardize_response=False):
    return wm.automatic_lambdas(x, y, mix, standardize, nlambda, ratio, standardize_response)


# ---- wmcov_cv_stats_kernel + wmcov_cv_assemble_kernel in numpy ----

def group_moments(x, y, fold, G, centre):
    """per group the (p + K + 1)^2 moments of [x - a | y - a_y | 1] about the whole-data centre, and that centre"""
    n, p = x.shape
    a = np.concatenate([x.mean(axis=0) if centre else np.zeros(p), y.mean(axis=0)])
    aug = np.column_stack([np.column_stack([x, y]) - a, np.ones(n)])
    return np.array([aug[fold == g].T @ aug[fold == g] for g in range(G)]), a


def pooled_problem(Cg, a, p, t, rest, standardize=True, centre=True, standardize_response=False):
    """what the two kernels leave for training set t (group t, or the total -- summed in group order -- less group t):
    dict(S ld x p column-major as (p, ld) rows = columns, diag, ct p x K, scale, mean p + K, yy, nulldev, nT)"""
    G, Pa = Cg.shape[0], Cg.shape[1]
    nc, K = Pa - 1, Pa - 1 - p
    C = Cg[t]
    if rest:
        total = np.zeros_like(C)
        for g in range(G):
            total = total + Cg[g]
        C = total - Cg[t]
    # stats: s, d, scale, mean, the responses' divisors, yy and the null deviance
    nT, s = C[nc, nc], C[:nc, nc].copy()
    d = s / nT
    if not centre:
        d[:p] = 0.0
    q = np.diag(C)[:nc] - d * s - d * s + nT * d * d
    v = q[:p] / nT
    scale = np.where(v > 0, np.sqrt(np.where(v > 0, v, 1.0)), 1.0) if standardize else np.ones(p)
    vy = q[p:] / nT
    ysd = np.where(vy > 0, np.sqrt(np.where(vy > 0, vy, 1.0)), 1.0) if standardize_response else np.ones(K)
    mean = np.concatenate([a[:p] + d[:p] if centre else np.zeros(p), np.zeros(K) if standardize_response else a[p:] + d[p:]])
    yy = nulldev = 0.0
    for r in range(K):
        nulldev += q[p + r]
        yy += q[p + r] / ysd[r] / ysd[r]
    # assemble: column j of S_T into the wide layout (rows p .. ld - 1 the zero pad), the smaller index first
    ld = leading_dim(p)
    S = np.zeros((p, ld))
    j, k = np.meshgrid(np.arange(p), np.arange(p), indexing="ij")
    lo, hi = np.minimum(j, k), np.maximum(j, k)
    S[:, :p] = (C[:p, :p] - d[lo] * s[hi] - d[hi] * s[lo] + nT * d[lo] * d[hi]) / nT / (scale[lo] * scale[hi])
    ct = (C[:p, p:nc] - d[:p, None] * s[None, p:] - d[None, p:] * s[:p, None] + nT * d[:p, None] * d[None, p:]) / ysd / nT / scale[:, None]
    return dict(S=S, diag=np.diag(S[:, :p]).copy(), ct=ct, scale=scale, mean=mean, yy=yy, nulldev=nulldev, nT=nT)


def direct_problem(x, y, standardize=True, centre=True, standardize_response=False):
    """the same from x[T], y[T] alone, as fit_mcovariance (driver_direct.cpp) prepares a single fit"""
    n, p = x.shape
    K = y.shape[1]
    mx, my = x.mean(axis=0), y.mean(axis=0)
    xc, yc = x - (mx if centre else 0.0), y - my
    v = ((x - mx) ** 2).mean(axis=0) if centre else (x ** 2).mean(axis=0)
    scale = np.where(v > 0, np.sqrt(np.where(v > 0, v, 1.0)), 1.0) if standardize else np.ones(p)
    vy = (yc ** 2).mean(axis=0)
    ysd = np.where(vy > 0, np.sqrt(np.where(vy > 0, vy, 1.0)), 1.0) if standardize_response else np.ones(K)
    xt, yt = xc / scale, yc / ysd
    S = xt.T @ xt / n
    return dict(S=S, diag=np.diag(S).copy(), ct=xt.T @ yt / n, scale=scale,
                mean=np.concatenate([mx if centre else np.zeros(p), np.zeros(K) if standardize_response else my]), yy=(yt ** 2).sum(),
                nulldev=(yc ** 2).sum(), nT=float(n))

"""Cross-validation in wide covariance mode (sa.cv_wcovariance_fits -> sgdnet_cv_wcovariance_*, sgdnet_amd/csrc/covariance.hip:
wcovariance_cv_run): the inputs and the numpy its tests share.  tests/test_gpu_cv_wcovariance.py runs them on the device,
tests/test_cv_wcovariance_host.py checks on the CPU what needs no device.  Inputs and numpy only: nothing here touches a GPU.

Tolerances (the project's own; none is derived from what the code under test returns)
  KKT_BOUND      1e-8   KKT residual <= 1e-8 * lambda (tests/test_gpu_covariance.py: assert_optimal)
  SAME_OPTIMUM   1e-9   "the same optimum reached twice", with the a0 rule of tests/test_gpu_cv_covariance.py: assert_same_fit
  POOLING_BOUND  1e-12  pooled against direct moments (tests/test_cv_covariance_host.py)"""
import numpy as np
import scipy.sparse as sp

import test_gpu_covariance as tc
import wcovariance_reference as wr

KKT_BOUND = tc.KKT_BOUND
SAME_OPTIMUM = 1e-9
POOLING_BOUND = 1e-12
TIGHT = dict(thresh=wr.THRESH, maxit=wr.MAXIT)
LIMIT = wr.LIMIT
MIXES = [0.0, 0.5, 1.0]

# (n, p, G); p = None: the feature limit.
#   (12, 1, 2)      one coordinate
#   (195, 15, 3)    groups of 65 rows, one past the 64-row stage
#   (192, 17, 3)    groups of exactly 64, p + 2 = 19 columns across the 16-column tile
#   (630, 199, 3)   the first p the narrow CV refuses; p odd (the last 16-byte slot is half pad); ld = 208 != p: the set stride
#   (660, 208, 3)   ld = p, no pad
#   (130, 257, 2)   one past a 256-lane stride, p > n_T
#   (130, 1025, 2)  the 1024-lane kernel with several jobs
#   (130, 1537, 2)  the first look-ahead instance with several jobs
#   (80, None, 2)   the feature limit (dense only, mix 0.5, 4 lambdas down to 0.1 lambda_max)
SHAPES = [(12, 1, 2), (195, 15, 3), (192, 17, 3), (630, 199, 3), (660, 208, 3), (130, 257, 2), (130, 1025, 2), (130, 1537, 2), (80, None, 2)]
MANY_JOBS = (90, 3, 90)          # leave-one-out, "rest", three mixes: 270 jobs on 256 compute units

# The byte budget of wcovariance_cv_run (csrc/covariance.hpp: kWcovCvBytes, wcov_cv_bytes); test_cv_wcovariance_host.py holds
# this copy against the constant the library reports in its refusal.
BUDGET_BYTES = 16 << 30


def leading_dim(p):
    return (p + 15) // 16 * 16


def tile_pairs(ncols):
    t = (ncols + 15) // 16
    return t * (t + 1) // 2


def rows_per_chunk(n, ncols, tile_rows=64):
    """csrc/wide_layout.hpp: wide_rows_per_chunk"""
    pairs = tile_pairs(ncols)
    cap = 1 if pairs >= 1024 else 1024 // pairs
    chunks = max(1, min((n + 255) // 256, cap))
    return ((n + chunks - 1) // chunks + tile_rows - 1) // tile_rows * tile_rows


def row_chunks(n, p, counts):
    """the dense group moments pass cuts its chunks at the groups' ends"""
    r = rows_per_chunk(n, p + 2)
    return int(sum((c + r - 1) // r for c in counts))


def budget_bytes(G, p, chunks):
    """group moments + their total + the dense partial tiles + the scaled matrices, in bytes (chunks = 0: sparse x)"""
    return 8 * ((G + 1) * (p + 2) ** 2 + chunks * tile_pairs(p + 2) * 256 + G * leading_dim(p) * p)


def groups_over_budget(p):
    """the fewest groups of one row each whose dense CV at p features is over the budget"""
    G = 1
    while budget_bytes(G, p, G) <= BUDGET_BYTES:
        G += 1
    return G


def path_of(p, mix):
    """(nlambda, lambda_min_ratio): wcovariance_reference.path_of, with its short paths (p > n) for every p from 257 on"""
    return wr.path_of(0, p if p is None or p < 257 else 257, mix)


def problem(n, p, sparse, seed=0):
    """tests/test_gpu_covariance.py: problem, with sparse x in a format that takes rows"""
    x, y = tc.problem(n, p, sparse, seed)
    return (sp.csr_matrix(x) if sparse else x), y


def equal_folds(n, G, seed=0):
    """labels 1..G in random order, sizes as equal as n allows (exactly n / G where G divides n)"""
    return np.random.default_rng(seed).permutation(np.arange(n) % G) + 1


def sorted_folds(x, G):
    """folds cut along sorted column 0: every fold's mean of it sits far from the whole-data mean the moments are centred at"""
    n = x.shape[0]
    col = np.asarray(x[:, 0].todense()).ravel() if sp.issparse(x) else x[:, 0]
    fold = np.empty(n, dtype=np.int64)
    fold[np.argsort(col, kind="stable")] = np.arange(n) * G // n
    return fold


def unequal_folds(n, seed=3):
    """four groups, labels that are not 1..G, one of them a single row"""
    sizes = [1, n // 3 - 1, n - 2 * (n // 3), n // 3]
    return np.repeat([10, 20, 30, 40], sizes)[np.random.default_rng(seed).permutation(n)]


def large_mean_problem(n, p, sparse):
    """problem() with column 2 of mean 1e6 and sd 1 (every entry stored) and a share of it in the response: the input of
    tests/test_gpu_cv_covariance.py: test_large_mean_column"""
    x, y = problem(n, p, sparse, seed=5)
    xd = np.asarray(x.todense()) if sparse else x.copy()
    col = np.random.default_rng(11).standard_normal(n)
    xd[:, 2] = 1e6 + (col - col.mean()) / col.std()
    return (sp.csr_matrix(xd) if sparse else xd), y + 0.7 * col


LARGE_MEAN_PATH = dict(nlambda=10, lambda_min_ratio=0.05)


def training_sets(foldid, train_on):
    return [(foldid == v) == (train_on == "fold") for v in np.unique(foldid)]


def lambdas(x, y, mix, standardize, nlambda, ratio):
    return wr.automatic_lambdas(x, y, mix, standardize, nlambda, ratio)

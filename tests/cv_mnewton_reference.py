"""What tests/test_cv_mnewton_host.py (CPU) and tests/test_gpu_cv_mnewton.py (GPU) share: the shapes, the folds, the pace
case and the numpy restatement of ONE job of the multinomial Newton cross-validation with its centres passed in.

A job solves x[T], y[T] as a Newton problem about fixed centres m (csrc/mnewton.hip).  The optimum does not depend on m; what
the iteration reaches at a given thresh could.  A separate fit takes m from the device's column sums (cov_sum_kernel: 256
lanes stride the rows, then a tree), the batched call from the host (driver_direct.cpp: the whole-data mean a plus the pooled
sum of x - a over T, divided by n_T): the same numbers but for rounding.  mnewton_path_about() is numpy_mnewton_path of
tests/test_gpu_mnewton.py with the centres passed in; device_order_centres() and host_order_centres() restate the two orders.

SAME_OPTIMUM, the relative distance the GPU test allows between a job and its separate fit, is the project's 1e-9
(tests/test_gpu_cv_covariance.py) while the measured cost of the centres (CENTRE_BOUND, test_cv_mnewton_host.py) stays at or
below 1e-10, as it did for the binomial cross-validation; it would be 10 x the measured value otherwise."""
import inspect

import numpy as np
import scipy.sparse as sp

import test_gpu_cv_covariance as tcv
import test_gpu_mnewton as tm

# the measured cost of the centres at thresh = 1e-12 over SMALL_SHAPES (test_cv_mnewton_host.py prints it per case): the
# largest was 4.91e-15 when the test was written; pinned at 10 x that, the margin the project gives its measured constants
# (the sums behind it are a BLAS's, whose order may differ between machines)
CENTRE_BOUND = 5e-14
SAME_OPTIMUM = tcv.SAME_OPTIMUM if CENTRE_BOUND <= 1e-10 else 10 * CENTRE_BOUND
assert SAME_OPTIMUM == 1e-9

MIXES = [0.0, 0.5, 1.0]
NLAMBDA, THRESH = 8, tm.THRESH
# (n, p, K, folds); p = None: mnewton_max_features(K)
SHAPES = [(45, 2, 3, 3),        # the smallest
          (192, 13, 3, 3),      # groups of 64: the 64-row staging step; p + 2 = 15
          (195, 14, 3, 3),      # groups of 65; p + 2 = 16, a tile edge
          (195, 15, 3, 3),      # p + 2 = 17
          (240, 14, 5, 3),      # Q = 75 > 64: the 256-lane inner solve
          (1003, 6, 4, 10)]     # 30 jobs; "rest" jobs open 4 row chunks, "fold" jobs 1, in one launch
LIMIT_SHAPES = [(300, None, 3, 3), (300, None, 2, 3)]      # one workgroup's LDS at the limit (Q = 198)
SMALL_SHAPES = SHAPES[:4]       # what the centre measurement runs on the CPU


def coefficients_are_unique(mix, K):
    """at mix = 1 and an even K the lasso optimum need not be unique in the coefficients (tests/test_gpu_mnewton.py): known
    from the parameters, never from the data"""
    return not (mix == 1.0 and K % 2 == 0)


def every_class_in_every_training_set(foldid, y, K, at_least=2):
    return all(np.bincount(y[T].astype(int), minlength=K).min() >= at_least for train_on in ("fold", "rest")
               for T in tcv.training_sets(foldid, train_on))


def folds(foldid, y, K):
    """foldid, after asserting that every training set -- each group and each complement -- holds every class, and twice:
    sgdnet_mnewton(), the separate fit a job is compared with, takes no class of one row"""
    assert every_class_in_every_training_set(foldid, y, K), "a training set with fewer than two rows of some class"
    return foldid


def equal_folds(n, G, y, K, seed=0):
    return folds(tcv.equal_folds(n, G, seed=seed), y, K)


def rows(x, T):
    return sp.csc_matrix(sp.csr_matrix(x)[T]) if sp.issparse(x) else x[T]


def lambdas(x, y, K, mix, standardize=True, nlambda=NLAMBDA, ratio=1e-2):
    """the driver's automatic path of the WHOLE data, handed to every job as user lambdas"""
    return tm.automatic_lambdas(x, y, K, mix, standardize, nlambda, ratio)


# ---- the pace case: a steep softmax signal and non-monotone user lambdas ----

STEEP_LAMBDAS = [2e-3, 5e-2, 5e-4]
STEEP = dict(n=195, p=5, K=3, folds=3, fold_seed=6, mixes=[0.5, 1.0])


def steep_problem(sparse):
    """n = 195, p = 5, K = 3 and a steep softmax signal: the Newton steps from lambda to lambda are long, and the jobs need
    different numbers of them"""
    n, p, K = STEEP["n"], STEEP["p"], STEEP["K"]
    rng = np.random.default_rng(42)
    x = rng.standard_normal((n, p)) * rng.uniform(0.5, 3.0, p) + rng.uniform(-2.0, 2.0, p)
    if sparse:
        keep = rng.random((n, p)) < 0.5
        keep[0, :] = True
        x = x * keep
    z = (x - x.mean(axis=0)) / x.std(axis=0)
    eta = np.column_stack([4.0 * z[:, 0] - 3.0 * z[:, 1] + 0.5, -4.0 * z[:, 0] + 2.0 * z[:, 2], 3.0 * z[:, 1] - 2.0 * z[:, 2] - 0.5])
    pr = np.exp(eta - eta.max(axis=1, keepdims=True))
    pr /= pr.sum(axis=1, keepdims=True)
    y = (pr.cumsum(axis=1) < rng.random(n)[:, None]).sum(axis=1).clip(0, K - 1).astype(float)
    return (sp.csc_matrix(x) if sparse else x), y


# ---- one job in numpy, its centres passed in ----

def mnewton_path_about(m, x, y, K, lam, mix, **kw):
    """numpy_mnewton_path (tests/test_gpu_mnewton.py) with the fixed centres of the Newton problem passed in: the source of
    that function with the one line that chooses them replaced, so that the two cannot drift apart."""
    src = inspect.getsource(tm.numpy_mnewton_path)
    line = "m = mean if (standardize or intercept) else np.zeros(p)"
    assert src.count(line) == 1 and src.count("def numpy_mnewton_path(") == 1
    src = src.replace(line, "m = np.asarray(CENTRES, dtype=float)").replace("def numpy_mnewton_path(", "def about(")
    scope = dict(vars(tm), CENTRES=m)
    exec(src, scope)
    return scope["about"](x, y, K, lam, mix, **kw)


def device_order_centres(xT):
    """cov_sum_kernel's order: lane t of 256 adds the rows t, t + 256, ... one by one, the lanes are joined by a tree"""
    xT = np.asarray(xT, dtype=float)
    lanes = np.zeros((256, xT.shape[1]))
    for i in range(xT.shape[0]):
        lanes[i % 256] += xT[i]
    width = 128
    while width:
        lanes[:width] += lanes[width:2 * width]
        width //= 2
    return lanes[0] / xT.shape[0]


def host_order_centres(x_all, foldid, value, train_on):
    """driver_direct.cpp's order: the whole-data mean a (one by one), per group the sum of x - a (one by one), the groups'
    sums added in group order (less the own group's when training on the rest), mean_T = a + S1 / n_T"""
    x_all = np.asarray(x_all, dtype=float)
    n = x_all.shape[0]
    a = np.zeros(x_all.shape[1])
    for i in range(n):
        a += x_all[i]
    a /= n
    values = np.unique(foldid)
    s1 = []
    for v in values:
        t = np.zeros(x_all.shape[1])
        for row in x_all[foldid == v]:
            t += row - a
        s1.append(t)
    total = np.zeros(x_all.shape[1])
    for t in s1:
        total += t
    own = s1[list(values).index(value)]
    n_own = int((foldid == value).sum())
    return a + ((own / n_own) if train_on == "fold" else (total - own) / (n - n_own))


def relative_distance(a0, beta, a0_ref, beta_ref):
    """coefficients relative to max|beta|, class-centred intercepts relative to max(1, max|a0|): the GPU test's measure"""
    return max(np.abs(beta - beta_ref).max() / np.abs(beta_ref).max(), np.abs(a0 - a0_ref).max() / max(1.0, np.abs(a0_ref).max()))

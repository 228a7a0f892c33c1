"""Cross-validation in wide Newton mode (sa.cv_wnewton_fits -> sgdnet_cv_wnewton_*, sgdnet_amd/csrc/newton.hip:
wnewton_cv_run): the shapes and inputs tests/test_gpu_cv_wnewton.py (device) and tests/test_cv_wnewton_host.py (CPU) share,
and the restatement of a job.

A job (mix, training set T) is BY DEFINITION wnewton_reference.numpy_wide_newton_path on x[T], y[T] (job_path).  The driver
does not take T's centres and scales from x[T]: it pools them from per-group sums of deviations about the whole-data column
means (driver_direct.cpp: sorted_dense_moments, pooled_centres_and_scales); pooled_job_path is the same restatement with the
centres and variances formed that way.

SHAPES (n, p, folds); p = None: the feature limit.
  (37, 2, 3)                                    the smallest call
  (192, 14, 3), (195, 15, 3), (195, 16, 3)      p + 2 around a 16-column tile; groups of 64 / 65 rows around a staged step
  (600, 199, 3)                                 the first p the narrow CV refuses
  (130, 255, 2), (130, 256, 2)                  P = p + 1 around one stride of 256 lanes and a bit word
  (130, 513, 2)                                 the first p the width rule gives 1024 lanes
  (130, 1024, 2)                                P one past a stride of 1024
  (80, None, 2)                                 the feature limit: one mix per case, KKT only
The lambdas are tn.automatic_lambdas of the whole data with wnewton_reference.path_of's length and ratio (6 values down to
1e-2 below p = 255; from there on, where the classes of a fold separate, 4 values down to 0.1 -- 1e-2 for ridge)."""
import inspect

import numpy as np
import scipy.sparse as sp

import test_gpu_cv_covariance as tcv
import test_gpu_newton as tn
import wnewton_reference as wr

KKT_BOUND = tn.KKT_BOUND
SAME_OPTIMUM = tcv.SAME_OPTIMUM
THRESH = wr.THRESH
MIXES = [0.0, 0.5, 1.0]
SHAPES = [(37, 2, 3), (192, 14, 3), (195, 15, 3), (195, 16, 3), (600, 199, 3), (130, 255, 2), (130, 256, 2), (130, 513, 2), (130, 1024, 2),
          (80, None, 2)]
COMPARE_UP_TO = 256                       # the separate fit of every job is compared up to this p (the cases stay short)
BOTH_MODES = [(195, 15, 3), (600, 198, 3)]                  # where the narrow CV runs too

equal_folds, training_sets = tcv.equal_folds, tcv.training_sets


def features(shape):
    return shape[1] or wr.LIMIT


def limit_mix(sparse, train_on):
    """at the feature limit one mix per case, rotated so that the four cases see all three (tests/test_gpu_cv_newton.py)"""
    return MIXES[(2 * sparse + (train_on == "rest") + 1) % 3]


def lambdas_of(x, y, shape, mix, standardize=True):
    nlambda, ratio = wr.path_of(shape[0], shape[1], mix)
    return tn.automatic_lambdas(x, y, mix, standardize, nlambda, ratio)


def dense(x):
    return np.asarray(x.todense()) if sp.issparse(x) else np.asarray(x, dtype=float)


# ---- the restatement of a job ----

def job_path(x, y, T, lam, mix, **kw):
    """the definition: the single wide fit on the rows of the training set"""
    return wr.numpy_wide_newton_path(dense(x)[T], y[T], lam, mix, **kw)


def pooled_moments(x, foldid, train_on):
    """per training set (in the order of np.unique(foldid)) the centres and variances as the driver pools them: per group the
    sums of d = x - a and of d^2 about the whole-data means a, the total added in group order, then
    mean_T = a + S1 / n_T and var_T = S2 / n_T - (S1 / n_T)^2"""
    xd = dense(x)
    a = xd.sum(axis=0) / xd.shape[0]
    groups = [foldid == v for v in np.unique(foldid)]
    s1 = [(xd[g] - a).sum(axis=0) for g in groups]
    s2 = [((xd[g] - a) ** 2).sum(axis=0) for g in groups]
    t1, t2 = np.zeros_like(a), np.zeros_like(a)
    for g in range(len(groups)):
        t1, t2 = t1 + s1[g], t2 + s2[g]
    out = []
    for g, own in enumerate(groups):
        nT = float(own.sum() if train_on == "fold" else (~own).sum())
        d = (s1[g] if train_on == "fold" else t1 - s1[g]) / nT
        var = (s2[g] if train_on == "fold" else t2 - s2[g]) / nT - d * d
        out.append((a + d, np.where(var > 0.0, var, 0.0)))
    return out


def pooled_job_path(x, y, T, moments, lam, mix, **kw):
    """numpy_wide_newton_path on x[T], y[T] with the centres and variances passed in: the source of that function with the two
    lines that form them replaced, so that the two cannot drift apart."""
    src = inspect.getsource(wr.numpy_wide_newton_path)
    lines = ("    mean = x.mean(axis=0)\n", "    var = ((x - mean) ** 2).mean(axis=0)\n")
    assert all(src.count(line) == 1 for line in lines) and src.count("def numpy_wide_newton_path(") == 1
    src = src.replace(lines[0], "    mean = np.asarray(POOLED[0], dtype=float)\n").replace(lines[1], "    var = np.asarray(POOLED[1], dtype=float)\n")
    scope = dict(vars(wr), POOLED=moments)
    exec(src.replace("def numpy_wide_newton_path(", "def pooled("), scope)
    return scope["pooled"](dense(x)[T], y[T], lam, mix, **kw)


def objective(a0, beta, xT, yT, lam, mix, standardize=True):
    """the penalised objective of the problem the driver solves on xT, yT (sgdnet_amd/kkt.py), per lambda: the mean binomial
    loss + lambda ((1 - mix) / 2 |w|^2 + mix |w|_1), w = beta x the standard deviations of xT"""
    xT = dense(xT)
    sd = xT.std(axis=0) if standardize else np.ones(xT.shape[1])
    sd = np.where(sd == 0, 1.0, sd)
    eta = xT @ beta + a0
    loss = (np.logaddexp(0.0, eta) - yT[:, None] * eta).mean(axis=0)
    w = beta * sd[:, None]
    return loss + lam * ((1 - mix) * 0.5 * (w ** 2).sum(axis=0) + mix * np.abs(w).sum(axis=0))


# ---- the row chunks of a job (csrc/wide_layout.hpp, restated) ----

TILE_ROWS = 64


def tile_pairs(ncols):
    t = (ncols + 15) // 16
    return t * (t + 1) // 2


def wide_row_chunks(n, ncols):
    pairs = tile_pairs(ncols)
    cap = 1 if pairs >= 1024 else 1024 // pairs
    return max(1, min((n + 255) // 256, cap))


def rows_per_chunk(n, ncols):
    c = wide_row_chunks(n, ncols)
    return ((n + c - 1) // c + TILE_ROWS - 1) // TILE_ROWS * TILE_ROWS


def job_chunks(n_t, p):
    """the chunks a single wide fit of n_t rows launches, which are the job's"""
    r = rows_per_chunk(n_t, p + 2)
    return (n_t + r - 1) // r


def row_chunk_inputs():
    """n = 500, p = 1.  'two': groups of 300 and 200 rows; train_on = "fold" puts a job of two row chunks beside a job of one
    (max_chunks > the second job's chunks).  With two groups the complement of a group is one range of rows, so 'gap' has three,
    of 100, 200 and 200 rows: train_on = "rest" gives the middle group's job the rows [0, 100) and [300, 500), and its first
    chunk of 192 local rows crosses from the one range into the other."""
    x, y = tn.problem(500, 1, False, seed=8)
    order = np.random.default_rng(8).permutation(500)
    out = {}
    for name, sizes in (("two", [300, 200]), ("gap", [100, 200, 200])):
        foldid = np.empty(500, dtype=np.int64)
        foldid[order] = np.repeat(np.arange(1, len(sizes) + 1), sizes)
        out[name] = (x, y, foldid, sizes)
    return out


def leave_one_out_input():
    """more jobs than compute units: leave-one-out over n = 90, p = 3 and three mixes is 270 jobs of 89 rows"""
    x, y = tn.problem(90, 3, False, seed=9)
    return x, y, np.arange(90)


# ---- halved steps ----

HALVING = dict(mix=0.5, lam=np.array([1e-6, 0.1]), thresh=1e-9, maxit=60)
# The relative difference of a job's penalised objective between the restatement about pooled centres and the one about the
# set's own, measured by tests/test_cv_wnewton_host.py::test_the_halving_input_halves_and_its_jobs_differ; the GPU test holds
# a job's objective to ten times it (floored at 1e-12) against the separate fit's.
HALVING_OBJECTIVE_DIFFERENCE = 1.65e-12
HALVING_OBJECTIVE_BOUND = max(10 * HALVING_OBJECTIVE_DIFFERENCE, 1e-12)


def halving_input():
    """Nearly separable data and a first lambda of 1e-6: the Newton steps towards it overshoot and are halved.  In the
    restatement (train_on = "rest", two folds) job 0 takes 18 + 7 steps with 1 halving and job 1 takes 20 + 7 steps with 4
    halvings; every lambda converges (tests/test_cv_wnewton_host.py asserts what of this the GPU test relies on)."""
    rng = np.random.default_rng(1)
    x = rng.standard_normal((120, 200))
    y = (x[:, 0] + 0.05 * rng.standard_normal(120) > 0).astype(float)
    return x, y, equal_folds(120, 2, seed=6)

#!/usr/bin/env python
"""Measurements of profiles/cv_wmcovariance.txt.

    PYTHONPATH=DIR python scripts/time_cv_wmcovariance.py separate|batched|single|bits [shape-index]

DIR holds the sgdnet_amd package to time: this checkout, or a build of the parent commit for `separate` and `bits`.  One
process times one (package, what); REPS timed calls (default 3) after one warm call; SGDNET_TRACE=1 adds the kernel times
(stderr).
  separate   the fold fits one by one (sgdnet_wmcovariance per training set + score): runs in the parent's tree too
  batched    cv_wmcovariance_fits + score, then the fold fits alone
  single     one job alone: sgdnet_wmcovariance on the training set of fold 0, every mix (with SGDNET_TRACE for kernel times)
  bits       sha256 of every array the single fits of wmcovariance_reference.inputs() return, and of one call each of
             cv_mcovariance_fits and cv_wcovariance_fits: what this change must leave alone
tests/ is this checkout's (files the parent has too)."""
import hashlib
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import torch  # noqa: F401,E402
import sgdnet_amd as sa  # noqa: E402

SHAPES = [(4000, 9, 3), (300, 174, 10), (2000, 1000, 3), (500, 3000, 2)]      # the shapes profiles/wmcovariance_path.txt has
MIXES = [0.1, 0.3, 0.5, 0.7, 1.0]
G, NLAMBDA = 10, 100


def problem(n, p, K):
    rng = np.random.default_rng(7 * n + 31 * p + K)
    x = rng.standard_normal((n, p)) * rng.uniform(0.5, 3.0, p) + rng.uniform(-2.0, 2.0, p)
    B = rng.standard_normal((p, K)) * (rng.random(p) < 0.1)[:, None]
    return x, x @ B + 0.5 * rng.standard_normal((n, K)) + rng.uniform(-2.0, 2.0, K)


def spread(ts):
    ts = np.array(ts)
    return "median %.3f s  min %.3f  max %.3f  (n = %d)" % (np.median(ts), ts.min(), ts.max(), ts.size)


def digest(fit):
    beta = fit.beta if isinstance(fit.beta, list) else [fit.beta]
    h = hashlib.sha256()
    for a in list(beta) + [fit.a0, fit.dev_ratio, fit.lambda_, fit.return_codes, fit.df]:
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(np.float64(fit.npasses).tobytes() + np.float64(fit.nulldev).tobytes())
    return h.hexdigest()[:32]


def bits():
    import test_gpu_cv_mcovariance as tcm
    import test_gpu_covariance as tc
    import wmcovariance_reference as wm
    for what, x, y, lam, mix, standardize, intercept, std_y in wm.inputs():
        fit = sa.sgdnet_wmcovariance(x, y, alpha=mix, lambda_=lam, standardize=standardize, intercept=intercept,
                                     standardize_response=std_y, thresh=wm.THRESH, maxit=wm.MAXIT)
        print("bits single", what, digest(fit), flush=True)
    for sparse in (False, True):
        x, y = tcm.problem(195, 13, 5, sparse)
        lam = [np.geomspace(1.0, 0.01, 6)] * 3
        for train_on in ("fold", "rest"):
            fits = sa.cv_mcovariance_fits(x, y, tcm.equal_folds(195, 3), [0.0, 0.5, 1.0], lam, train_on=train_on, thresh=1e-12, maxit=1000000)
            for job, fit in enumerate(fits):
                print("bits cv_mcovariance", sparse, train_on, job, digest(fit), flush=True)
        x, y = tc.problem(630, 199, sparse)
        x = sp.csr_matrix(x) if sparse else x
        for train_on in ("fold", "rest"):
            fits = sa.cv_wcovariance_fits(x, y, tcm.equal_folds(630, 3), [0.0, 0.5, 1.0], lam, train_on=train_on, thresh=1e-12, maxit=1000000)
            for job, fit in enumerate(fits):
                print("bits cv_wcovariance", sparse, train_on, job, digest(fit), flush=True)


def main():
    what = sys.argv[1]
    print("library:", sa.LIB_PATH, flush=True)
    if what == "bits":
        return bits()
    shapes = [SHAPES[int(sys.argv[2])]] if len(sys.argv) > 2 else SHAPES
    reps = int(os.environ.get("REPS", "3"))
    for n, p, K in shapes:
        x, y = problem(n, p, K)
        foldid = np.random.default_rng(1).permutation(np.arange(n) % G)
        lam = [sa.sgdnet_wmcovariance(x, y, alpha=m, nlambda=NLAMBDA).lambda_ for m in MIXES]
        sets = [foldid != g for g in range(G)]

        def separate():
            out = []
            for a, m in enumerate(MIXES):
                for T in sets:
                    fit = sa.sgdnet_wmcovariance(x[T], y[T], alpha=m, lambda_=lam[a])
                    out.append(sa.score(fit, x[~T], y[~T], "deviance"))
            return out

        def batched():
            fits = sa.cv_wmcovariance_fits(x, y, foldid, MIXES, lam, train_on="rest")
            return [sa.score(fits[a * G + j], x[~T], y[~T], "deviance") for a in range(len(MIXES)) for j, T in enumerate(sets)]

        def batched_fits_only():
            return sa.cv_wmcovariance_fits(x, y, foldid, MIXES, lam, train_on="rest")

        def single():
            return [sa.sgdnet_wmcovariance(x[sets[0]], y[sets[0]], alpha=m, lambda_=lam[a]) for a, m in enumerate(MIXES)]

        runs = {"separate": [separate], "batched": [batched, batched_fits_only], "single": [single]}[what]
        for f in runs:
            f()                                   # warm
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                res = f()
                ts.append(time.perf_counter() - t0)
            print("%s %d x %d, K = %d, %d mixes x %d folds, %d lambdas: %s" % (f.__name__, n, p, K, len(MIXES), G, NLAMBDA, spread(ts)),
                  flush=True)
            if f.__name__ in ("separate", "batched"):
                print("   mean held-out deviance over all jobs and lambdas: %.12g" % np.mean(res), flush=True)


main()

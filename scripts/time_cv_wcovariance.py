#!/usr/bin/env python
"""Measurements of profiles/cv_wcovariance.txt.

    PYTHONPATH=DIR python scripts/time_cv_wcovariance.py separate|batched|single|bits [shape-index]

DIR holds the sgdnet_amd package to time: this checkout, or a build of the parent commit for `separate` and `bits`.  One
process times one (package, what); REPS timed calls (default 3) after one warm call; SGDNET_TRACE=1 adds the kernel times
(stderr).
  separate   the fold fits one by one (sgdnet_wcovariance per training set + score): runs in the parent's tree too
  batched    cv_wcovariance_fits + score
  single     one job alone: sgdnet_wcovariance on the training set of fold 0, every mix (with SGDNET_TRACE for kernel times)
  bits       sha256 of the single fits of wcovariance_reference.SHAPES x dense/sparse at mix 0.5
tests/ is this checkout's (files the parent has too)."""
import hashlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import torch  # noqa: F401,E402
import sgdnet_amd as sa  # noqa: E402

SHAPES = [(4177, 198), (2000, 1000), (20000, 1000), (500, 3000)]
MIXES = [0.1, 0.3, 0.5, 0.7, 1.0]
G, NLAMBDA = 10, 100


def problem(n, p):
    rng = np.random.default_rng(7 * n + p)
    x = rng.standard_normal((n, p)) * rng.uniform(0.5, 3.0, p) + rng.uniform(-2.0, 2.0, p)
    B = rng.standard_normal(p) * (rng.random(p) < 0.1)
    return x, x @ B + 0.5 * rng.standard_normal(n) + 1.5


def spread(ts):
    ts = np.array(ts)
    return "median %.3f s  min %.3f  max %.3f  (n = %d)" % (np.median(ts), ts.min(), ts.max(), ts.size)


def main():
    what = sys.argv[1]
    print("library:", sa.LIB_PATH, flush=True)
    if what == "bits":
        import test_gpu_covariance as tc
        import wcovariance_reference as wr
        for n, p in wr.SHAPES:
            for sparse in (False, True):
                pp = p or sa.wcovariance_max_features()
                x, y = tc.problem(n, pp, sparse)
                nl, ratio = wr.path_of(n, p, 0.5)
                fit = sa.sgdnet_wcovariance(x, y, alpha=0.5, nlambda=nl, lambda_min_ratio=ratio, thresh=wr.THRESH, maxit=wr.MAXIT)
                h = hashlib.sha256(fit.beta.tobytes() + np.asarray(fit.a0).tobytes() + fit.dev_ratio.tobytes() + fit.lambda_.tobytes()).hexdigest()
                print("bits", (n, pp), "sparse" if sparse else "dense", h[:32], "npasses %g" % fit.npasses, flush=True)
        return
    shapes = [SHAPES[int(sys.argv[2])]] if len(sys.argv) > 2 else SHAPES
    reps = int(os.environ.get("REPS", "3"))
    for n, p in shapes:
        x, y = problem(n, p)
        foldid = np.random.default_rng(1).permutation(np.arange(n) % G)
        lam = [sa.sgdnet_wcovariance(x, y, alpha=m, nlambda=NLAMBDA).lambda_ for m in MIXES]
        sets = [foldid != g for g in range(G)]

        def separate():
            out = []
            for a, m in enumerate(MIXES):
                for T in sets:
                    fit = sa.sgdnet_wcovariance(x[T], y[T], alpha=m, lambda_=lam[a])
                    out.append(sa.score(fit, x[~T], y[~T], "deviance"))
            return out

        def batched():
            fits = sa.cv_wcovariance_fits(x, y, foldid, MIXES, lam, train_on="rest")
            return [sa.score(fits[a * G + j], x[~T], y[~T], "deviance") for a in range(len(MIXES)) for j, T in enumerate(sets)]

        def batched_fits_only():
            return sa.cv_wcovariance_fits(x, y, foldid, MIXES, lam, train_on="rest")

        def single():
            return [sa.sgdnet_wcovariance(x[sets[0]], y[sets[0]], alpha=m, lambda_=lam[a]) for a, m in enumerate(MIXES)]

        runs = {"separate": [separate], "batched": [batched, batched_fits_only], "single": [single]}[what]
        for f in runs:
            f()                                   # warm
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                res = f()
                ts.append(time.perf_counter() - t0)
            print("%s %d x %d, %d mixes x %d folds, %d lambdas: %s" % (f.__name__, n, p, len(MIXES), G, NLAMBDA, spread(ts)), flush=True)
            if f.__name__ in ("separate", "batched"):
                print("   mean held-out deviance over all jobs and lambdas: %.12g" % np.mean(res), flush=True)


main()

#!/usr/bin/env python
"""Wall time of a multinomial cross-validation whose fits are sgdnet_mnewton(): fold fits one by one against
fold_fits="batched" (profiles/cv_mnewton.txt, by the protocol of profiles/cv_mcovariance.txt).

    python scripts/time_cv_mnewton.py --package DIR --route separate|batched --workload iris|k10 [--timed N]

--package: the directory that holds the sgdnet_amd package to time (this checkout by default; a build of the parent commit
for its separate route).  One process times one (package, route, workload): run the two builds alternately in fresh processes.
  separate   the package's own _cv() (full fits, fold fits on x[T], y[T], score()) with sa.sgdnet_mnewton injected as the
             fit: what cv_sgdnet_mnewton(fold_fits="separate") is, and runs on a build that has no cv_sgdnet_mnewton
  batched    sa.cv_sgdnet_mnewton(fold_fits="batched")
Workloads: iris (150 x 4, K = 3) and problem(2000, 18, 10) of tests/test_gpu_mnewton.py (K = 10 at its feature limit);
alpha = [0, .25, .5, .75, 1], 10 folds of equal size in which every class has two rows or more, train_on = "fold", 100
lambdas, default thresh.  Two warm-up calls, then median / min / max of N timed calls; behind the bar the single fit
sa.sgdnet_mnewton(alpha = 0.5) and, where the package has it, sa.cv_mnewton_fits alone (the 50 fold fits with the full fits'
lambdas).  Run once more with SGDNET_TRACE=1 for the rounds of the lock-step loop (stderr)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHAS = [0.0, 0.25, 0.5, 0.75, 1.0]
NFOLDS, NLAMBDA = 10, 100


def workload(name):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_mnewton as tm
    x, y = tm.iris() if name == "iris" else tm.problem(2000, 18, 10)
    K = int(y.max()) + 1
    for seed in range(100):                                     # the first equal folds in which every class has two rows or more
        foldid = np.random.default_rng(seed).permutation(np.arange(len(y)) % NFOLDS) + 1
        if all(np.bincount(y[foldid == v].astype(int), minlength=K).min() >= 2 for v in range(1, NFOLDS + 1)):
            return x, y, foldid, seed
    raise SystemExit("no fold seed below 100 puts two rows of every class into every fold")


def stats(f, timed, warm=2):
    for _ in range(warm):
        f()
    t = []
    for _ in range(timed):
        t0 = time.perf_counter()
        out = f()
        t.append(1e3 * (time.perf_counter() - t0))
        print("  call %.1f ms" % t[-1], file=sys.stderr, flush=True)
    return "median %.3f ms min %.3f max %.3f (n=%d)" % (np.median(t), min(t), max(t), len(t)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=ROOT)
    ap.add_argument("--route", choices=["separate", "batched"], required=True)
    ap.add_argument("--workload", choices=["iris", "k10"], required=True)
    ap.add_argument("--timed", type=int, default=5)
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    import sgdnet_amd as sa
    from sgdnet_amd import cv as sacv
    assert os.path.dirname(os.path.dirname(os.path.abspath(sa.__file__))) == os.path.abspath(args.package), sa.__file__
    x, y, foldid, fold_seed = workload(args.workload)

    def separate():
        def fit_one(xx, yy, lam, a, dev, fit_seed, rng, sequential):
            return sa.sgdnet_mnewton(xx, yy, alpha=float(a), lambda_=lam, nlambda=NLAMBDA, device=dev)
        return sacv._cv(x, y, ALPHAS, None, NFOLDS, foldid, "deviance", family="multinomial", devices=[0], rng=None, seed=0,
                        train_on="fold", densify=False, fit_one=fit_one, batched_fits=None)

    def batched():
        return sa.cv_sgdnet_mnewton(x, y, alpha=ALPHAS, foldid=foldid, nlambda=NLAMBDA, fold_fits="batched")

    whole, cv = stats(separate if args.route == "separate" else batched, args.timed)
    single, _ = stats(lambda: sa.sgdnet_mnewton(x, y, alpha=0.5, nlambda=NLAMBDA), 4 * args.timed)
    line = "%s %dx%d K=%d cv fold_fits=%s: %s | single fit alpha=0.5: %s | lambda_min %g alpha_min %g" % (
        args.label or os.path.basename(os.path.abspath(args.package)), x.shape[0], x.shape[1], int(y.max()) + 1, args.route, whole, single,
        cv.lambda_min, cv.alpha_min)
    if hasattr(sa, "cv_mnewton_fits"):
        alone, fits = stats(lambda: sa.cv_mnewton_fits(x, y, foldid, ALPHAS, cv.lambda_), args.timed)
        line += " | cv_mnewton_fits (%d jobs) alone: %s; steps + halvings of the slowest job %d" % (
            len(fits), alone, max(f.diagnostics["steps"] + f.diagnostics["halvings"] for f in fits))
    print(line + " | fold seed %d" % fold_seed, flush=True)


if __name__ == "__main__":
    main()

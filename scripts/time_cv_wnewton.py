#!/usr/bin/env python
"""Wall time of a binomial cross-validation whose fits are sgdnet_wnewton(): fold fits one by one against
fold_fits="batched" (profiles/cv_wnewton.txt).

    python scripts/time_cv_wnewton.py --shape 2000x1000 [--timed N] [--warm W] [--out FILE]

One process times one shape, both routes in it, alternating (separate, batched, separate, ...): the separate route is
cv_sgdnet_wnewton(fold_fits="separate"), one sgdnet_wnewton per fold, the code the mode had before it had a batched CV.
Workload: tests/test_gpu_newton.py's problem(n, p) (dense, binomial), alpha = [0.1, 0.3, 0.5, 0.7, 1.0], 10 folds of equal size,
train_on = "rest", 100 lambdas (those of the full fits, which both routes run alike), default thresh and maxit.  The shapes of
profiles/cv_wcovariance.txt: 4177x198, 2000x1000, 20000x1000, 500x3000.
W warm-up rounds of both routes, then median / min / max of N timed calls each, wall clock around the Python call (every call
ends in a device synchronise).  Then the 50 fold fits alone (sa.cv_wnewton_fits with the full fits' lambdas), and one more
such call under SGDNET_TRACE=1 for the library's line: jobs, rounds, the slowest job, sweeps, and the kernel times per phase
(moments / scale / inner solves / state; hipEvent times, which cost nothing extra here: a round ends in a synchronise anyway).
The mean held-out deviance over all folds, mixes and lambdas is printed per route to show both computed the same thing."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHAS = [0.1, 0.3, 0.5, 0.7, 1.0]
NFOLDS, NLAMBDA = 10, 100


def stats(t):
    return "median %.3f s  min %.3f  max %.3f  (n = %d)" % (np.median(t), min(t), max(t), len(t))


def traced(f):
    """f() with SGDNET_TRACE=1 and the library's stderr lines returned"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["SGDNET_TRACE"] = "1"
        try:
            out = f()
        finally:
            del os.environ["SGDNET_TRACE"]
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return out, tmp.read().decode(errors="replace").splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", required=True, help="NxP")
    ap.add_argument("--timed", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--out", default=None, help="append the report to this file as well")
    args = ap.parse_args()
    n, p = (int(v) for v in args.shape.split("x"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sgdnet_amd as sa
    import test_gpu_newton as tn
    if sa.load().sgdnet_device_count() < 1:
        raise SystemExit("time_cv_wnewton.py needs a HIP device: a time taken elsewhere says nothing")
    x, y = tn.problem(n, p, False)
    foldid = np.random.default_rng(0).permutation(np.arange(n) % NFOLDS) + 1
    kw = dict(alpha=ALPHAS, foldid=foldid, nlambda=NLAMBDA, train_on="rest")
    routes = {r: (lambda r=r: sa.cv_sgdnet_wnewton(x, y, fold_fits=r, **kw)) for r in ("separate", "batched")}

    report = []

    def say(line):
        print(line, flush=True)
        report.append(line)

    times = {r: [] for r in routes}
    cv = {}
    for i in range(args.warm + args.timed):
        for r, f in routes.items():
            t0 = time.perf_counter()
            cv[r] = f()
            dt = time.perf_counter() - t0
            print("  %s call %d: %.3f s%s" % (r, i, dt, " (warm-up)" if i < args.warm else ""), file=sys.stderr, flush=True)
            if i >= args.warm:
                times[r].append(dt)
    head = "%d x %d, %d mixes x %d folds, %d lambdas" % (n, p, len(ALPHAS), NFOLDS, NLAMBDA)
    for r in routes:
        say("  %s %s: %s" % (r, head, stats(times[r])))
        say("     mean held-out deviance over all jobs and lambdas: %.12g" % np.mean([np.mean(m) for m in cv[r].cv_raw]))
    lam = cv["batched"].lambda_
    fits_only = lambda: sa.cv_wnewton_fits(x, y, foldid, ALPHAS, lam, train_on="rest")        # noqa: E731
    t = []
    for i in range(args.warm + args.timed):
        t0 = time.perf_counter()
        fits = fits_only()
        if i >= args.warm:
            t.append(time.perf_counter() - t0)
    say("  batched_fits_only %s: %s" % (head, stats(t)))
    say("     unconverged lambdas over all jobs: %d; steps + halvings of the slowest job %d"
        % (int(sum((f.return_codes != 0).sum() for f in fits)), max(f.diagnostics["steps"] + f.diagnostics["halvings"] for f in fits)))
    _, lines = traced(fits_only)
    for line in lines:
        if "cv wnewton" in line:
            say("    " + line.replace("[sgdnet]", "").strip())
    med = {r: float(np.median(times[r])) for r in routes}
    say("  %s: separate / batched (whole CV) = %.2f: batched is %s" % (args.shape, med["separate"] / med["batched"],
                                                                     "faster" if med["batched"] < med["separate"] else "slower there"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(report) + "\n")


if __name__ == "__main__":
    main()

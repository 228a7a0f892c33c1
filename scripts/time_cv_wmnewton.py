#!/usr/bin/env python
"""Wall time of a multinomial cross-validation whose fits are sgdnet_wmnewton(): fold fits one by one against
fold_fits="batched" under both settings of the option "cv_wmnewton_moments" (profiles/cv_wmnewton.txt).

    python scripts/time_cv_wmnewton.py --shape 2000x1000x3 [--timed N] [--warm W] [--out FILE] [--moments 0|1|both] [--no-separate]

One process times one shape (n x p x K), all routes in it, alternating (separate, batched at 0, batched at 1, separate, ...):
the separate route is cv_sgdnet_wmnewton(fold_fits="separate"), one sgdnet_wmnewton per fold, the only route the mode had.
Workload: tests/test_gpu_mnewton.py's problem(n, p, K) (dense, multinomial), alpha = [0.1, 0.3, 0.5, 0.7, 1.0], 10 folds of equal
size, train_on = "rest", 100 lambdas (those of the full fits, which all routes run alike), default thresh and maxit.  The shapes
of profiles/wmnewton_path.txt: 300x66x3, 2000x1000x3, 500x2500x2, 20000x200x10.
W warm-up rounds of every route, then median / min / max of N timed calls each, wall clock around the Python call (every call
ends in a device synchronise).  Then the 50 fold fits alone (sa.cv_wmnewton_fits with the full fits' lambdas) under each
setting, and one more such call under SGDNET_TRACE=1 for the library's line: jobs, rounds, the slowest job, sweeps, the moments
kernel and moments_ms / scale_ms / cd_ms / state_ms (hipEvent times, which cost nothing extra here: a round ends in a
synchronise anyway).  The mean held-out deviance over all folds, mixes and lambdas is printed per route to show all computed
the same thing."""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_cv_wnewton import stats, traced  # noqa: E402

ALPHAS = [0.1, 0.3, 0.5, 0.7, 1.0]
NFOLDS, NLAMBDA = 10, 100
OPTION = "cv_wmnewton_moments"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", required=True, help="NxPxK")
    ap.add_argument("--timed", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--out", default=None, help="append the report to this file as well")
    ap.add_argument("--moments", default="both", choices=["0", "1", "both"], help='the option "cv_wmnewton_moments" of the batched route')
    ap.add_argument("--no-separate", action="store_true", help="leave the separate route out")
    args = ap.parse_args()
    n, p, K = (int(v) for v in args.shape.split("x"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sgdnet_amd as sa
    import test_gpu_mnewton as tm
    if sa.load().sgdnet_device_count() < 1:
        raise SystemExit("time_cv_wmnewton.py needs a HIP device: a time taken elsewhere says nothing")
    x, y = tm.problem(n, p, K, False)
    foldid = np.random.default_rng(0).permutation(np.arange(n) % NFOLDS) + 1
    kw = dict(alpha=ALPHAS, foldid=foldid, nlambda=NLAMBDA, train_on="rest")
    settings = (0, 1) if args.moments == "both" else (int(args.moments),)

    def under(setting, f):
        def call():
            with sa.option(OPTION, setting):
                return f()
        return call

    routes = {} if args.no_separate else {"separate": lambda: sa.cv_sgdnet_wmnewton(x, y, fold_fits="separate", **kw)}
    for m in settings:
        routes["batched, moments = %d" % m] = under(m, lambda: sa.cv_sgdnet_wmnewton(x, y, fold_fits="batched", **kw))

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
    head = "%d x %d, K = %d, %d mixes x %d folds, %d lambdas" % (n, p, K, len(ALPHAS), NFOLDS, NLAMBDA)
    for r in routes:
        say("  %s %s: %s" % (r, head, stats(times[r])))
        say("     mean held-out deviance over all jobs and lambdas: %.12g" % np.mean([np.mean(m) for m in cv[r].cv_raw]))
    lam = next(iter(cv.values())).lambda_
    only = {m: under(m, lambda: sa.cv_wmnewton_fits(x, y, foldid, ALPHAS, lam, train_on="rest")) for m in settings}
    t, fits = {m: [] for m in settings}, {}
    for i in range(args.warm + args.timed):
        for m in settings:
            t0 = time.perf_counter()
            fits[m] = only[m]()
            if i >= args.warm:
                t[m].append(time.perf_counter() - t0)
    for m in settings:
        say("  batched_fits_only, moments = %d %s: %s" % (m, head, stats(t[m])))
        say("     unconverged lambdas over all jobs: %d; steps + halvings of the slowest job %d"
            % (int(sum((f.return_codes != 0).sum() for f in fits[m])),
               max(f.diagnostics["steps"] + f.diagnostics["halvings"] for f in fits[m])))
        say("     sha256 of every job's coefficients and intercepts: %s"
            % hashlib.sha256(b"".join(np.stack(f.beta).tobytes() + f.a0.tobytes() for f in fits[m])).hexdigest()[:16])
        _, lines = traced(only[m])
        for line in lines:
            if "cv wmnewton:" in line:
                say("    " + line.replace("[sgdnet]", "").strip())
    med = {r: float(np.median(times[r])) for r in routes}
    for m in settings:
        if "separate" in med:
            b = med["batched, moments = %d" % m]
            say("  %s: separate / batched at moments = %d (whole CV) = %.2f: batched is %s" % (args.shape, m, med["separate"] / b,
                                                                                            "faster" if b < med["separate"] else "slower there"))
    if len(settings) == 2:
        say("  %s: fold fits alone, moments 0 / moments 1 = %.2f" % (args.shape, np.median(t[0]) / np.median(t[1])))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(report) + "\n")


if __name__ == "__main__":
    main()

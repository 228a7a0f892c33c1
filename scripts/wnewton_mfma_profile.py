"""Times of sa.sgdnet_wnewton behind profiles/wnewton_mfma.txt: the moments pass by the tile kernel (the option
"wnewton_moments" = 0) and by the matrix-core kernel (1), alternating in one process; scripts/wnewton_profile.py's inputs and
path (binomial, alpha = 0.5, 100 lambdas, the default thresh).  Per setting: one warm-up fit, then rounds of timed fits (wall
time of the call), then fits under SGDNET_TRACE for the split from the library's HIP events (fits of their own: the events cost
a synchronise per step).  A library from another commit is timed by the same script: SGDNET_LIB_PATH=... --moments 0.
Needs a GPU.

    python scripts/wnewton_mfma_profile.py --moments 0,1 [--auto] 4177x198 20000x1000 500x2000 500x4000 2> trace.txt
"""
import argparse
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np

import sgdnet_amd as sa
import test_gpu_newton as tn

KW = dict(alpha=0.5, nlambda=100)


def fit_with(setting, x, y):
    if setting == "auto":
        return sa.sgdnet(x, y, family="binomial", mode="auto", **KW)
    if setting == "as built":                                # a library without the option
        return sa.sgdnet_wnewton(x, y, **KW)
    with sa.option("wnewton_moments", int(setting)):
        return sa.sgdnet_wnewton(x, y, **KW)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--moments", default="0,1", help="the option's values to time, or 'none' for a library without it")
    ap.add_argument("--auto", action="store_true", help="also time mode = auto (once)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-fits", type=int, default=1, help="fits under SGDNET_TRACE after the timed ones (rocprofv3 runs: 0)")
    ap.add_argument("shapes", nargs="+")
    args = ap.parse_args()
    if sa.load().sgdnet_device_count() < 1:
        raise SystemExit("wnewton_mfma_profile.py needs a HIP device")
    settings = ["as built"] if args.moments == "none" else args.moments.split(",")
    lib = os.environ.get("SGDNET_LIB_PATH", "this build")
    for arg in args.shapes:
        n, p = (int(v) for v in arg.split("x"))
        x, y = tn.problem(n, p, False)
        os.environ.pop("SGDNET_TRACE", None)
        for setting in settings + (["auto"] if args.auto else []):
            fit_with(setting, x, y)
        times = {s: [] for s in settings}
        fits = {}
        for _ in range(args.rounds):
            for setting in settings:
                for _ in range(2):
                    t0 = time.perf_counter()
                    fits[setting] = fit_with(setting, x, y)    # (returns after the coefficients are on the host)
                    times[setting].append(time.perf_counter() - t0)
        if args.auto:
            times["auto"] = []
            for _ in range(2):
                t0 = time.perf_counter()
                fits["auto"] = fit_with("auto", x, y)
                times["auto"].append(time.perf_counter() - t0)
        for setting, ts in times.items():
            fit = fits[setting]
            print("%s | %d x %d moments %-8s median %.4f s min %.4f max %.4f (n=%d) npasses %g dev_ratio[-1] %.6f unconverged %d kkt ratio max %.3g "
                  "digest %s" % (lib, n, p, setting, statistics.median(ts), min(ts), max(ts), len(ts), fit.npasses, fit.dev_ratio[-1],
                                 int((fit.return_codes != 0).sum()), float(np.max(sa.kkt(fit, x, y)["ratio"])),
                                 hashlib.sha256(fit.beta.tobytes() + fit.a0.tobytes()).hexdigest()[:16]), flush=True)
        os.environ["SGDNET_TRACE"] = "1"
        for _ in range(args.trace_fits):
            for setting in settings:
                print("trace %s | %d x %d moments %s:" % (lib, n, p, setting), file=sys.stderr, flush=True)
                fit_with(setting, x, y)
        os.environ.pop("SGDNET_TRACE", None)


if __name__ == "__main__":
    main()

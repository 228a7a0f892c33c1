"""Times of sa.sgdnet_wmnewton behind profiles/wmnewton_mfma.txt: the class-pair moments pass by the tile kernel (the option
"wmnewton_moments" = 0) and by the matrix-core kernel (1), alternating in one process; scripts/wmnewton_profile.py's inputs and
path (multinomial, alpha = 0.5, 100 lambdas, the default thresh).  Per setting: one warm-up fit, then rounds of timed fits (wall
time of the call), then fits under SGDNET_TRACE for the split from the library's HIP events (fits of their own: the events cost
a synchronise per step).  A library from another commit is timed by the same script: SGDNET_LIB_PATH=... --moments none.  The
digest of beta and a0 says whether two libraries returned the same bits.  A shape is n x p x K; one process per shape.
Needs a GPU.

    python scripts/wmnewton_mfma_profile.py --moments 0,1 [--auto] 20000x200x10 2> trace.txt
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
import test_gpu_mnewton as tm
from wmnewton_profile import fit_with as fit_other

KW = dict(alpha=0.5, nlambda=100)


def fit_with(setting, x, y):
    if setting == "auto":
        return fit_other("auto", x, y)
    if setting == "as built":                                # a library without the option
        return sa.sgdnet_wmnewton(x, y, **KW)
    with sa.option("wmnewton_moments", int(setting)):
        return sa.sgdnet_wmnewton(x, y, **KW)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--moments", default="0,1", help="the option's values to time, or 'none' for a library without it")
    ap.add_argument("--auto", action="store_true", help="also time mode = auto")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of two timed fits per setting")
    ap.add_argument("--trace-fits", type=int, default=1, help="fits under SGDNET_TRACE after the timed ones")
    ap.add_argument("shapes", nargs="+")
    args = ap.parse_args()
    if sa.load().sgdnet_device_count() < 1:
        raise SystemExit("wmnewton_mfma_profile.py needs a HIP device")
    settings = ["as built"] if args.moments == "none" else args.moments.split(",")
    other = os.environ.get("SGDNET_LIB_PATH")                # named by its directory: .../parent/libsgdnet_hip.so is "parent"
    lib = "%-10s" % (os.path.basename(os.path.dirname(other)) if other else "this build")
    for arg in args.shapes:
        if arg == "iris":
            (x, y), K = tm.iris(), 3
        else:
            n, p, K = (int(v) for v in arg.split("x"))
            x, y = tm.problem(n, p, K)
        n, p = x.shape
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
            for _ in range(3):
                t0 = time.perf_counter()
                fits["auto"] = fit_with("auto", x, y)
                times["auto"].append(time.perf_counter() - t0)
        for setting, ts in times.items():
            fit = fits[setting]
            print("%s | %d x %d K=%d moments %-8s median %.4f s min %.4f max %.4f (n=%d) npasses %g dev_ratio[-1] %.6f unconverged %d "
                  "kkt ratio max %.3g digest %s" % (lib, n, p, K, setting, statistics.median(ts), min(ts), max(ts), len(ts), fit.npasses,
                                                    fit.dev_ratio[-1], int((fit.return_codes != 0).sum()),
                                                    float(np.max(sa.kkt(fit, x, y)["ratio"])),
                                                    hashlib.sha256(tm.stacked(fit).tobytes() + np.asarray(fit.a0).tobytes()).hexdigest()[:16]),
                  flush=True)
        os.environ["SGDNET_TRACE"] = "1"
        for _ in range(args.trace_fits):
            for setting in settings:
                print("trace %s | %d x %d K=%d moments %s:" % (lib, n, p, K, setting), file=sys.stderr, flush=True)
                fit_with(setting, x, y)
        os.environ.pop("SGDNET_TRACE", None)


if __name__ == "__main__":
    main()

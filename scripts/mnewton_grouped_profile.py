"""Times of the grouped multinomial penalty behind profiles/mnewton_grouped.txt: sa.sgdnet_mnewton (where it takes the shape)
and sa.sgdnet_wmnewton with type_multinomial="grouped" against the same mode ungrouped and against mode = "auto" with the
grouped penalty, alternating in one process.  Multinomial, alpha = 0.5, the 100-lambda path at the default thresh.  Per
setting: one warm-up fit, then rounds of timed fits (wall time of the call, which returns after the coefficients are on the
host), the worst KKT ratio of the penalty the fit was made with, then one fit under SGDNET_TRACE for the inner sweeps (stderr).
A shape is n x p x K; "iris" is the 150 x 4 data set of the tests (K = 3).  Needs a GPU.

    python scripts/mnewton_grouped_profile.py iris 300x65x3 2000x1000x3 20000x200x10 2> trace.txt
"""
import argparse
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

KW = dict(alpha=0.5, nlambda=100)


def fit_with(setting, x, y):
    mode, penalty = setting.split("/")
    if mode == "auto":
        # through the shared front end (scripts/wmnewton_profile.py).  No public entry point offers the grouped penalty in
        # mode = "auto": api._fit sends type_multinomial = 1 and holds "mnewton_grouped" at 1 meanwhile, which SAGA does not read.
        from sgdnet_amd import _lib, api
        return api._fit(x, y, "multinomial", KW["alpha"], KW["nlambda"], None, None, 1000, True, True, 0.001, False, debug=False, seed=0,
                        rng=None, sample_stream=None, unif=None, mode="auto", modes=_lib.MODES, batch=0, device=0, devices=None,
                        min_classes=2, type_multinomial=penalty)
    return getattr(sa, "sgdnet_" + mode)(x, y, type_multinomial=penalty, **KW)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="timed fits per setting")
    ap.add_argument("shapes", nargs="+")
    args = ap.parse_args()
    if sa.load().sgdnet_device_count() < 1:
        raise SystemExit("mnewton_grouped_profile.py needs a HIP device")
    for arg in args.shapes:
        if arg == "iris":
            (x, y), K = tm.iris(), 3
        else:
            n, p, K = (int(v) for v in arg.split("x"))
            x, y = tm.problem(n, p, K)
        n, p = x.shape
        modes = (["mnewton"] if p <= sa.mnewton_max_features(K) else []) + ["wmnewton"]
        settings = [m + "/" + pen for m in modes for pen in ("grouped", "ungrouped")] + ["auto/grouped"]
        os.environ.pop("SGDNET_TRACE", None)
        for setting in settings:
            fit_with(setting, x, y)
        times, fits = {s: [] for s in settings}, {}
        for _ in range(args.rounds):
            for setting in settings:
                t0 = time.perf_counter()
                fits[setting] = fit_with(setting, x, y)
                times[setting].append(time.perf_counter() - t0)
        for setting, ts in times.items():
            fit = fits[setting]
            ratio = float(np.max(sa.kkt(fit, x, y, grouped=setting.endswith("/grouped"))["ratio"]))
            print("%d x %d K=%d %-18s median %.4f s min %.4f max %.4f (n=%d) npasses %g dev_ratio[-1] %.6f unconverged %d kkt ratio max %.3g"
                  % (n, p, K, setting, statistics.median(ts), min(ts), max(ts), len(ts), fit.npasses, fit.dev_ratio[-1],
                     int((fit.return_codes != 0).sum()), ratio), flush=True)
        os.environ["SGDNET_TRACE"] = "1"
        for setting in settings[:-1]:
            print("trace %d x %d K=%d %s:" % (n, p, K, setting), file=sys.stderr, flush=True)
            fit_with(setting, x, y)
        os.environ.pop("SGDNET_TRACE", None)


if __name__ == "__main__":
    main()

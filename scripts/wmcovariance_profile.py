"""Times of sa.sgdnet_wmcovariance (SGDNET_MODE_WMCOVARIANCE) behind profiles/wmcovariance_path.txt: the wall time of the
call against sa.sgdnet_mcovariance (where it takes the shape) or sa.sgdnet(family="mgaussian", mode="auto"), the split into
moments / scale / path kernel from the library's HIP events (SGDNET_TRACE), the list sweeps, both widths of the path
kernel's workgroup, and both modes' worst KKT ratio.  mgaussian, alpha = 0.5, the 100-lambda path at the default thresh.
Needs a GPU.

    python scripts/wmcovariance_profile.py 300x174x10 4000x9x3 2000x1000x3 500x3000x2 2> trace.txt
"""
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
import test_gpu_mcovariance as tm

KW = dict(alpha=0.5, nlambda=100)


def fit_with(setting, x, y, **kw):
    kw = dict(KW, **kw)
    if setting == "mcovariance":
        return sa.sgdnet_mcovariance(x, y, **kw)
    if setting == "auto":
        return sa.sgdnet(x, y, family="mgaussian", mode="auto", **kw)
    with sa.option("wmcovariance_width", {"rule": 0, "w256": 256, "w1024": 1024}[setting]):
        return sa.sgdnet_wmcovariance(x, y, **kw)


def main():
    if sa.load().sgdnet_device_count() < 1:
        raise SystemExit("wmcovariance_profile.py needs a HIP device")
    for arg in sys.argv[1:]:
        n, p, K = (int(v) for v in arg.split("x"))
        x, y = tm.problem(n, p, K, False)
        other = "mcovariance" if p <= sa.mcovariance_max_features(K) else "auto"
        settings = ["rule", "w256", "w1024", other]
        os.environ.pop("SGDNET_TRACE", None)
        for setting in settings:                          # warm-up: code objects, allocations (auto: a short path)
            fit_with(setting, x, y, **(dict(nlambda=3) if setting == "auto" else {}))
        for rnd in range(2):
            for setting in settings:
                if setting == "auto" and rnd:
                    continue
                times = []
                for _ in range(3 if setting != "auto" else 1):
                    t0 = time.perf_counter()
                    fit = fit_with(setting, x, y)         # (returns after the coefficients are on the host)
                    times.append(time.perf_counter() - t0)
                ratio = float(np.max(sa.kkt(fit, x, y)["ratio"]))
                digest = hashlib.sha256(tm.stacked(fit).tobytes() + fit.a0.tobytes()).hexdigest()[:16]
                print("%d x %d K %d %-11s median %.4f s min %.4f max %.4f (n=%d) npasses %g dev_ratio[-1] %.6f unconverged %d kkt ratio max %.3g digest %s"
                      % (n, p, K, setting, statistics.median(times), min(times), max(times), len(times), fit.npasses, fit.dev_ratio[-1],
                         int((fit.return_codes != 0).sum()), ratio, digest), flush=True)
        # the split: the library's events, from fits that are not the timed ones
        os.environ["SGDNET_TRACE"] = "1"
        for setting in settings:
            if setting == "auto":
                continue
            print("trace %d x %d K %d %s:" % (n, p, K, setting), file=sys.stderr, flush=True)
            for _ in range(2):
                fit_with(setting, x, y)
        os.environ.pop("SGDNET_TRACE", None)


if __name__ == "__main__":
    main()

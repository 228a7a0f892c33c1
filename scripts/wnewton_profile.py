"""Times of sa.sgdnet_wnewton (SGDNET_MODE_WNEWTON) behind profiles/wnewton_path.txt: the wall time of the call against
sa.sgdnet_newton (where it takes the shape) or sa.sgdnet(mode="auto"), the split into state / moments / scale / inner solve
from the library's HIP events (SGDNET_TRACE), the outer steps and sweeps, both widths of the inner solve's workgroup, and
both modes' worst KKT ratio.  Binomial, alpha = 0.5, the 100-lambda path at the default thresh.  Needs a GPU.

    python scripts/wnewton_profile.py 4177x198 20000x1000 500x2000 500x4000 2> trace.txt
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
import test_gpu_newton as tn

KW = dict(alpha=0.5, nlambda=100)


def fit_with(setting, x, y):
    if setting == "newton":
        return sa.sgdnet_newton(x, y, **KW)
    if setting == "auto":
        return sa.sgdnet(x, y, family="binomial", mode="auto", **KW)
    with sa.option("wnewton_width", {"rule": 0, "w256": 256, "w1024": 1024}[setting]):
        return sa.sgdnet_wnewton(x, y, **KW)


def main():
    if sa.load().sgdnet_device_count() < 1:
        raise SystemExit("wnewton_profile.py needs a HIP device")
    for arg in sys.argv[1:]:
        n, p = (int(v) for v in arg.split("x"))
        x, y = tn.problem(n, p, False)
        other = "newton" if p <= sa.newton_max_features() else "auto"
        settings = ["rule", "w256", "w1024"] + ([other] if p != 2000 else [])
        os.environ.pop("SGDNET_TRACE", None)
        for setting in settings:                          # warm-up: code objects, allocations
            fit_with(setting, x, y)
        for rnd in range(2):
            for setting in settings:
                if setting == "auto" and rnd:
                    continue
                times = []
                for _ in range(3 if setting != "auto" else 2):
                    t0 = time.perf_counter()
                    fit = fit_with(setting, x, y)         # (returns after the coefficients are on the host)
                    times.append(time.perf_counter() - t0)
                ratio = float(np.max(sa.kkt(fit, x, y)["ratio"]))
                digest = hashlib.sha256(fit.beta.tobytes() + fit.a0.tobytes()).hexdigest()[:16]
                print("%d x %d %-6s median %.4f s min %.4f max %.4f (n=%d) npasses %g dev_ratio[-1] %.6f unconverged %d kkt ratio max %.3g digest %s"
                      % (n, p, setting, statistics.median(times), min(times), max(times), len(times), fit.npasses, fit.dev_ratio[-1],
                         int((fit.return_codes != 0).sum()), ratio, digest), flush=True)
        # the split: the library's events cost a synchronise per step, so these fits are not the timed ones
        os.environ["SGDNET_TRACE"] = "1"
        for setting in settings:
            if setting == "auto":
                continue
            print("trace %d x %d %s:" % (n, p, setting), file=sys.stderr, flush=True)
            for _ in range(2):
                fit_with(setting, x, y)
        os.environ.pop("SGDNET_TRACE", None)


if __name__ == "__main__":
    main()

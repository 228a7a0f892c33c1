"""Times of sa.sgdnet_wmnewton (SGDNET_MODE_WMNEWTON) behind profiles/wmnewton_path.txt: the wall time of the call against
sa.sgdnet_mnewton (where it takes the shape) or sa.sgdnet(family="multinomial", mode="auto"), the split into state /
moments / scale / inner solve from the library's HIP events (SGDNET_TRACE), the outer steps and sweeps, both widths of the
inner solve's workgroup, and both fits' worst KKT ratio.  Multinomial, alpha = 0.5, the 100-lambda path at the default
thresh.  A shape is n x p x K; "iris" is the 150 x 4 data set of the tests (K = 3).  Needs a GPU.

    python scripts/wmnewton_profile.py iris 300x65x3 20000x200x10 2000x1000x3 500x2500x2 2> trace.txt
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
import test_gpu_mnewton as tm

KW = dict(alpha=0.5, nlambda=100)
RUNS = 5


def fit_with(setting, x, y):
    if setting == "mnewton":
        return sa.sgdnet_mnewton(x, y, **KW)
    if setting == "auto":
        # sa.sgdnet(family="multinomial", mode="auto") through the shared front end: sgdnet() itself sends a response of
        # two classes to family = "binomial", which is another problem (one coefficient vector, half the penalty)
        from sgdnet_amd import _lib, api
        return api._fit(x, y, "multinomial", KW["alpha"], KW["nlambda"], None, None, 1000, True, True, 0.001, False, debug=False, seed=0,
                        rng=None, sample_stream=None, unif=None, mode="auto", modes=_lib.MODES, batch=0, device=0, devices=None,
                        min_classes=2)
    with sa.option("wmnewton_width", {"rule": 0, "w256": 256, "w1024": 1024}[setting]):
        return sa.sgdnet_wmnewton(x, y, **KW)


def main():
    if sa.load().sgdnet_device_count() < 1:
        raise SystemExit("wmnewton_profile.py needs a HIP device")
    for arg in sys.argv[1:]:
        if arg == "iris":
            (x, y), K = tm.iris(), 3
        else:
            n, p, K = (int(v) for v in arg.split("x"))
            x, y = tm.problem(n, p, K)
        n, p = x.shape
        other = "mnewton" if p <= sa.mnewton_max_features(K) else "auto"
        settings = ["rule", "w256", "w1024", other]
        os.environ.pop("SGDNET_TRACE", None)
        for setting in settings:                          # warm-up: code objects, allocations
            fit_with(setting, x, y)
        for setting in settings:
            times = []
            for _ in range(RUNS):
                t0 = time.perf_counter()
                fit = fit_with(setting, x, y)             # (returns after the coefficients are on the host)
                times.append(time.perf_counter() - t0)
            ratio = float(np.max(sa.kkt(fit, x, y)["ratio"]))
            digest = hashlib.sha256(tm.stacked(fit).tobytes() + np.asarray(fit.a0).tobytes()).hexdigest()[:16]
            print("%d x %d K=%d %-7s median %.4f s min %.4f max %.4f (n=%d) npasses %g dev_ratio[-1] %.6f unconverged %d kkt ratio max %.3g digest %s"
                  % (n, p, K, setting, statistics.median(times), min(times), max(times), len(times), fit.npasses, fit.dev_ratio[-1],
                     int((fit.return_codes != 0).sum()), ratio, digest), flush=True)
        # the split: the library's events cost a synchronise per step, so these fits are not the timed ones
        os.environ["SGDNET_TRACE"] = "1"
        for setting in settings:
            if setting == "auto":
                continue
            print("trace %d x %d K=%d %s:" % (n, p, K, setting), file=sys.stderr, flush=True)
            for _ in range(2):
                fit_with(setting, x, y)
        os.environ.pop("SGDNET_TRACE", None)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time sa.path_gradient at BASELINE config 3's shape (1M x 1000, 1 % non-zeros, binomial, 100 lambdas) next to the
numpy host pass it replaces.  Run under `rocprofv3 --kernel-trace --stats -- python scripts/gradient_timing.py` for the
device time of the kernels; the wall times printed here include the upload of x.

    python scripts/gradient_timing.py [--n 1000000] [--p 1000] [--nlambda 100]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=1_000)
    ap.add_argument("--nlambda", type=int, default=100)
    args = ap.parse_args()
    import sgdnet_amd as sa
    from sgdnet_amd import data as D
    pr = D.make_sparse_glm(args.n, args.p, 0.01, family="binomial", seed=3)
    xs = D.as_scipy(pr).T.tocsc()                 # samples in rows, as sgdnet() takes it
    y = pr["y"].ravel()
    rng = np.random.default_rng(0)
    L = args.nlambda
    beta = np.asfortranarray(0.1 * rng.standard_normal((1, args.p, L)) * (rng.random((1, args.p, L)) < 0.3))
    a0 = np.asfortranarray(0.1 * rng.standard_normal((1, L)))
    fit = SimpleNamespace(family="binomial", a0=a0, beta=beta)
    sa.path_gradient(fit, xs[:1000], y[:1000])    # load the library, create the context
    t0 = time.time()
    G, G0 = sa.path_gradient(fit, xs, y)
    t_dev = time.time() - t0
    t0 = time.time()
    xr = xs.tocsr()
    r = 1.0 - y[:, None] - 1.0 / (1.0 + np.exp(xr @ beta[0] + a0))
    Gn = (xs.T @ r) / args.n
    G0n = r.mean(axis=0)
    t_host = time.time() - t0
    print(json.dumps({"shape": [args.n, args.p, L], "nnz": int(xs.nnz), "path_gradient_wall_s": t_dev, "numpy_host_pass_s": t_host,
                      "max_abs_diff": float(max(np.abs(G[0] - Gn).max(), np.abs(G0[0] - G0n).max()))}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""The launches of the covariance-family runs (sgdnet_amd/csrc/covariance.hip), for comparing two builds of the library.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python scripts/covariance_launch_sequence.py run
    python scripts/covariance_launch_sequence.py list DIR            # the ordered (kernel, grid, workgroup, LDS) of a trace

`run` calls, in one process and at tiny shapes, every fit (covariance, wcovariance, mcovariance, wmcovariance) with dense and
with sparse x, and every cross-validated form with dense and sparse x, once with train_on="fold" and once with "rest".
SGDNET_LIB_PATH picks the library (sgdnet_amd/_lib.py); profiles/covariance_host_fold.txt has the lists of two builds."""
import csv
import glob
import os
import sys


def run():
    import numpy as np
    import scipy.sparse as sp
    import torch  # noqa: F401
    import sgdnet_amd as sa
    print("library:", sa.LIB_PATH, flush=True)
    rng = np.random.default_rng(0)
    n, p, K, G = 300, 5, 2, 2
    x = rng.standard_normal((n, p)) * (rng.random((n, p)) < 0.5)
    x[0] = 1.0
    Y = x[:, :K] + 0.5 * rng.standard_normal((n, K))
    foldid = np.repeat([1, 2], [250, 50])[rng.permutation(n)]           # dense x: the first group spans two row chunks
    lam = np.array([0.1, 0.01])
    for xs in (x, sp.csr_matrix(x)):
        sa.sgdnet(xs, Y[:, 0], alpha=0.5, lambda_=lam, mode="covariance")
        sa.sgdnet_wcovariance(xs, Y[:, 0], alpha=0.5, lambda_=lam)
        sa.sgdnet_mcovariance(xs, Y, alpha=0.5, lambda_=lam)
        sa.sgdnet_wmcovariance(xs, Y, alpha=0.5, lambda_=lam)
        for train_on in ("fold", "rest"):
            sa.cv_covariance_fits(xs, Y[:, 0], foldid, [0.5, 1.0], [lam, lam], train_on=train_on)
            sa.cv_wcovariance_fits(xs, Y[:, 0], foldid, [0.5, 1.0], [lam, lam], train_on=train_on)
            sa.cv_mcovariance_fits(xs, Y, foldid, [0.5, 1.0], [lam, lam], train_on=train_on)
            sa.cv_wmcovariance_fits(xs, Y, foldid, [0.5, 1.0], [lam, lam], train_on=train_on)
    print("done", flush=True)


def launches(directory):
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    dims = lambda r, what: "x".join(r["%s_%s" % (what, d)] for d in "XYZ")       # noqa: E731
    lds = "LDS_Block_Size" if "LDS_Block_Size" in rows[0] else "Group_Segment_Size"
    return ["%s grid %s workgroup %s lds %s" % (r["Kernel_Name"], dims(r, "Grid_Size"), dims(r, "Workgroup_Size"), r[lds]) for r in rows]


if __name__ == "__main__":
    if sys.argv[1:2] == ["list"]:
        print("\n".join(launches(sys.argv[2])))
    else:
        run()

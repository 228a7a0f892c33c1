"""Cross-validation in wide covariance mode (sgdnet_cv_wcovariance_*, sgdnet_amd/csrc/covariance.hip: wcovariance_cv_run), the
parts a CPU can check: the refusals of the native entry points that are decided before a device is looked for, the argument
checks of cv_sgdnet_wcovariance, the byte budget's arithmetic, and what the pooling of the moments costs at the wide shapes.

The pooling check is tests/test_cv_covariance_host.py's (pooled_problem against direct_problem, bound 1e-12) at the shapes
of tests/cv_wcovariance_reference.py, (90, 3, 90) on "rest" only; all three (standardize, centre) settings up to 208 features,
the default beyond.  Measured with those functions when this test was written: the largest relative difference over all
shapes was 3.4e-15 -- the reference alone stays more than two orders of magnitude inside the bound."""
import ctypes as C
import re

import numpy as np
import pytest

import cv_wcovariance_reference as cr
import test_cv_covariance_host as th


def test_pooled_moments_are_the_direct_ones_at_the_wide_shapes():
    worst = 0.0
    for n, p, G in cr.SHAPES + [cr.MANY_JOBS]:
        p = p or cr.LIMIT
        x, y = th.problem(n, p)
        fold = th.random_folds(n, G)
        settings = ((True, True), (False, True), (False, False)) if p <= 208 else ((True, True),)
        for rest in ((True,) if (n, p, G) == cr.MANY_JOBS else (False, True)):
            for standardize, centre in settings:
                for t in range(G):
                    T = (fold != t) if rest else (fold == t)
                    S, c = th.pooled_problem(x, y, fold, G, t, rest, standardize, centre)
                    S0, c0 = th.direct_problem(x[T], y[T], standardize, centre)
                    err = max(np.abs(S - S0).max() / np.abs(S0).max(), np.abs(c - c0).max() / max(np.abs(c0).max(), 1e-300))
                    worst = max(worst, err)
                    assert err <= cr.POOLING_BOUND, (n, p, G, rest, standardize, centre, t, err)
    print("pooled vs direct S / c~ at the wide shapes: largest relative difference %.3g" % worst)


def test_budget_arithmetic():
    """csrc/covariance.hpp: kWcovCvBytes and the examples of its comment"""
    assert cr.BUDGET_BYTES == 16 * 2 ** 30
    ten, twenty = cr.budget_bytes(10, cr.LIMIT, 10), cr.budget_bytes(20, cr.LIMIT, 20)
    assert ten <= cr.BUDGET_BYTES and twenty <= cr.BUDGET_BYTES                     # a 10-fold CV at the limit fits
    assert round(ten / 1e9, 2) == 4.28 and round(twenty / 1e9, 2) == 8.40
    # at the limit the tile pairs alone are 1024 workgroups and more: one row chunk per group whatever n is
    assert cr.tile_pairs(cr.LIMIT + 2) == 40470 and cr.row_chunks(10 ** 6, cr.LIMIT, [10 ** 5] * 10) == 10
    assert cr.budget_bytes(849, 1000, 849) <= cr.BUDGET_BYTES < cr.budget_bytes(850, 1000, 850) and cr.groups_over_budget(1000) == 850
    # sparse x has no partial tiles
    assert cr.budget_bytes(10, cr.LIMIT, 0) == ten - 8 * 10 * 40470 * 256


def test_native_refusals_name_the_condition():
    import scipy.sparse as sp

    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    rng = np.random.default_rng(0)
    limit = sa.wcovariance_max_features()
    assert limit == cr.LIMIT

    def refused(code, needle, x, y, foldid):
        with pytest.raises(sa.SgdnetError) as e:
            sa.cv_wcovariance_fits(x, y, foldid, 0.5, np.array([0.1, 0.01]))
        assert e.value.code == code and needle in str(e.value), str(e.value)
        return str(e.value)

    wide = rng.standard_normal((6, limit + 1))
    refused(-5, "mode = wcovariance needs no more features than sgdnet_wcovariance_max_features()", wide, wide[:, 0], np.arange(6) % 3)
    refused(-5, "mode = wcovariance needs no more features", sp.csc_matrix(wide), wide[:, 0], np.arange(6) % 3)
    # the byte budget, from the constant: the fewest one-row groups that are over it at 1000 features (x itself is 6.8 MB)
    p = 1000
    G = cr.groups_over_budget(p)
    big = rng.standard_normal((G, p))
    msg = refused(-5, "mode = wcovariance needs the moments and the scaled matrices of the groups within %d bytes" % cr.BUDGET_BYTES, big,
                  big[:, 0], np.arange(G))
    assert int(re.search(r"are (\d+) bytes", msg).group(1)) == cr.budget_bytes(G, p, G) > cr.BUDGET_BYTES      # the message gives the bytes
    # ... one group fewer is within it: the call gets as far as looking for a device or running
    assert cr.budget_bytes(G - 1, p, G - 1) <= cr.BUDGET_BYTES
    # the narrow CV refuses what it always refused, by its own name
    x199 = rng.standard_normal((30, 199))
    with pytest.raises(sa.SgdnetError, match="mode = covariance needs no more features"):
        sa.cv_covariance_fits(x199, x199[:, 0], np.arange(30) % 3, 0.5, np.array([0.1, 0.01]))

    # what cv_wcovariance_fits cannot express goes through the C ABI directly
    L = sa.load()
    x = rng.standard_normal((60, 4))
    y = x[:, 0] + rng.standard_normal(60)
    xf, yf, f32 = np.asfortranarray(x), np.ascontiguousarray(y), np.ascontiguousarray(np.arange(60) % 3, dtype=np.int32)

    def call(fold_arr=f32, n_groups=3, lam_arr=np.array([[0.1, 0.01]]), alphas=np.array([0.5]), train_on_rest=0, **ctl_fields):
        ctl = _lib.Control()
        ctl.family, ctl.intercept, ctl.standardize, ctl.max_iter, ctl.tol, ctl.n_lambda, ctl.n_classes = 0, 1, 1, 100, 1e-7, 2, 1
        ctl.mode = _lib.MODE_WCOVARIANCE
        for k, v in ctl_fields.items():
            setattr(ctl, k, v)
        out = [np.zeros(3 * 2), np.zeros(3 * 2 * 4), np.zeros(3 * 2), np.zeros(3 * 2), np.zeros(3), np.zeros(3)]
        res = _lib.CvCovResult(*[_lib.dptr(a) for a in out])
        rc = L.sgdnet_cv_wcovariance_dense(_lib.dptr(xf), 60, 4, _lib.dptr(yf), fold_arr.ctypes.data_as(C.POINTER(C.c_int32)), n_groups,
                                           train_on_rest, C.byref(ctl), 1, _lib.dptr(alphas), _lib.dptr(lam_arr), C.byref(res))
        return rc, L.sgdnet_last_error().decode()

    rc, msg = call(n_gpus=2)
    assert rc == -5 and msg.startswith("mode = wcovariance needs one GPU"), msg
    rc, msg = call(debug=1)
    assert rc == -5 and msg.startswith("mode = wcovariance needs debug = 0"), msg
    rc, msg = call(family=1)
    assert rc == -5 and msg.startswith("mode = wcovariance needs family = gaussian"), msg
    bad = f32.copy()
    bad[7] = 3
    rc, msg = call(fold_arr=bad)
    assert rc == -1 and "fold[7] = 3" in msg, msg
    bad[7] = -1
    rc, msg = call(fold_arr=bad)
    assert rc == -1 and "fold[7] = -1" in msg, msg
    rc, msg = call(n_groups=4)
    assert rc == -1 and "group 3 of 4 is empty" in msg, msg
    rc, msg = call(lam_arr=np.array([[0.1, -0.01]]))
    assert rc == -1 and "negative" in msg, msg
    for mix in (-0.1, 1.5, np.nan):
        rc, msg = call(alphas=np.array([mix]))
        assert rc == -1 and "not an elastic-net mix in [0, 1]" in msg, msg
    rc, msg = call(fold_arr=np.zeros(60, dtype=np.int32), n_groups=1, train_on_rest=1)
    assert rc == -1 and "sgdnet_cv_wcovariance" in msg and "train_on_rest needs two groups" in msg, msg


def test_python_argument_checks():
    import sgdnet_amd as sa
    assert "cv_wcovariance_fits" in sa.__all__ and "cv_sgdnet_wcovariance" in sa.__all__
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = x[:, 0] + rng.standard_normal(60)
    for needle, kw in (("'separate' or 'batched'", dict(fold_fits="fused")), ("'fold' or 'rest'", dict(train_on="others")),
                       ("'fold' or 'rest'", dict(train_on="others", fold_fits="batched"))):
        with pytest.raises(ValueError) as e:
            sa.cv_sgdnet_wcovariance(x, y, nfolds=3, **kw)
        assert needle in str(e.value), str(e.value)
    with pytest.raises(TypeError):
        sa.cv_sgdnet_wcovariance(x, y, nfolds=3, mode="covariance")                           # the mode is not an argument
    with pytest.raises(ValueError):
        sa.cv_wcovariance_fits(x, y, np.arange(60) % 3, [0.5, 1.0], [[0.1, 0.01]])            # one lambda array per alpha
    with pytest.raises(ValueError):
        sa.cv_wcovariance_fits(x, y, np.arange(60) % 3, 0.5, [0.1, -0.01])
    with pytest.raises(ValueError):
        sa.cv_wcovariance_fits(x, y, np.arange(60) % 3, 1.5, [0.1, 0.01])
    with pytest.raises(ValueError):
        sa.cv_wcovariance_fits(x, y, np.arange(60) % 3, 0.5, [0.1], train_on="others")
    with pytest.raises(ValueError):
        sa.cv_wcovariance_fits(x, y[:-1], np.arange(60) % 3, 0.5, [0.1])
    # cv_sgdnet(fold_fits="batched") stays covariance mode's alone
    with pytest.raises(ValueError, match="mode='covariance'"):
        sa.cv_sgdnet(x, y, nfolds=3, fold_fits="batched", mode="wcovariance")

"""Cross-validation in wide multi-response covariance mode (sgdnet_cv_wmcovariance_*, sgdnet_amd/csrc/covariance.hip:
wmcovariance_cv_run), the parts a CPU can check: that the entry points exist, the refusals that are decided before a device
is looked for, the byte budget's arithmetic against the constant the library prints, a numpy restatement of
wmcov_cv_stats_kernel + wmcov_cv_assemble_kernel against the directly computed problem of x[T], y[T], and that the inputs
of the GPU test admit its KKT bound (the numpy restatement of the path kernel reaches it on every training set).

Measured when this test was written: pooled against direct over the small shapes 2.9e-15 (S, c~, scale, mean, yy and the
null deviance, relative; 1.2e-15 with the column of mean 1e6); worst KKT ratio of the restatement 5.1e-11, intercept
residual 1.5e-13 lambda."""
import ctypes as C
import re

import numpy as np
import pytest

import cv_wmcovariance_reference as cr
import wmcovariance_reference as wm


def test_the_entry_points_exist():
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    L = sa.load()
    for name in ("sgdnet_cv_wmcovariance_dense", "sgdnet_cv_wmcovariance_sparse"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert "cv_wmcovariance_fits" in sa.__all__ and "cv_sgdnet_wmcovariance" in sa.__all__
    assert callable(sa.cv_wmcovariance_fits) and callable(sa.cv_sgdnet_wmcovariance)
    assert L.sgdnet_abi_version() == 6                      # additions only


def difference(got, ref, p):
    rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)       # noqa: E731
    assert (got["S"][:, p:] == 0.0).all() and got["nT"] == ref["nT"]            # the zero pad; n_T is a count
    assert got["S"][:, :p].tobytes() == got["S"][:, :p].T.copy().tobytes()      # symmetric bit for bit
    return max(rel(got["S"][:, :p], ref["S"]), rel(got["diag"], ref["diag"]), rel(got["ct"], ref["ct"]), rel(got["scale"], ref["scale"]),
               rel(got["mean"], ref["mean"]), abs(got["yy"] - ref["yy"]) / ref["yy"], abs(got["nulldev"] - ref["nulldev"]) / ref["nulldev"])


SETTINGS = ((True, True, False), (False, True, False), (False, False, False), (True, True, True))   # (standardize, centre, standardize_response)


def test_pooled_stats_and_assembly_are_the_direct_problem():
    worst = worst_mean = 0.0
    for n, p, K, G in cr.SMALL_SHAPES:
        inputs = [(cr.problem(n, p, K, False), cr.equal_folds(n, G) - 1)]
        x, y = cr.problem(n, p, K, False, seed=3)
        inputs.append(((x, y), cr.sorted_folds(x, G)))
        if p > 2:
            inputs.append((cr.large_mean_problem(n, p, K, False), cr.equal_folds(n, G, seed=6) - 1))
        for which, ((x, y), fold) in enumerate(inputs):
            for standardize, centre, std_y in SETTINGS:
                if which == 2 and not centre:
                    # uncentred features: c~_j = sum_i x_ij (y_i - mean y) / n with x_ij = 1e6 + O(1) cancels seven digits in the
                    # direct computation just as in the pooled one (they differ by 1.3e-10): there is no reference to hold
                    continue
                Cg, a = cr.group_moments(x, y, fold, G, centre)
                for rest in (False, True):
                    for t in range(G):
                        T = (fold != t) if rest else (fold == t)
                        err = difference(cr.pooled_problem(Cg, a, p, t, rest, standardize, centre, std_y),
                                         cr.direct_problem(x[T], y[T], standardize, centre, std_y), p)
                        if which == 2:
                            worst_mean = max(worst_mean, err)
                        else:
                            worst = max(worst, err)
                        assert err <= cr.POOLING_BOUND, (n, p, K, G, which, rest, standardize, centre, std_y, t, err)
    print("pooled vs direct: largest relative difference %.3g (column of mean 1e6: %.3g)" % (worst, worst_mean))


def test_the_inputs_admit_the_kkt_bound():
    """wmcovariance_reference.numpy_wide_group_path on every training set of the small shapes: the bound the GPU test holds
    every job to is reachable on these inputs at its thresh"""
    worst = worst_a0 = 0.0
    for n, p, K, G in cr.SMALL_SHAPES:
        x, y = cr.problem(n, p, K, False)
        foldid = cr.equal_folds(n, G)
        for mix in cr.MIXES:
            lam = cr.lambdas(x, y, mix, True, *cr.path_of(n, p, G))
            for train_on in ("fold", "rest"):
                for T in cr.training_sets(foldid, train_on):
                    a0, beta, _, sweeps, _, _, unconverged = wm.numpy_wide_group_path(x[T], y[T], lam, mix)
                    assert not unconverged.any() and sweeps.max() < wm.MAXIT
                    k = wm.numpy_kkt(a0, beta, x[T], y[T], lam, mix, True, True)
                    worst, worst_a0 = max(worst, np.max(k["ratio"])), max(worst_a0, np.max(k["intercept"] / lam))
                    assert (k["ratio"] <= cr.KKT_BOUND).all() and (k["intercept"] <= cr.KKT_BOUND * lam).all(), (n, p, K, mix, train_on)
    print("worst KKT ratio of the restatement %.3g, intercept residual %.3g lambda" % (worst, worst_a0))


def test_budget_arithmetic():
    """csrc/covariance.hpp: wmcov_cv_bytes within kWcovCvBytes and the examples of its comment"""
    assert cr.BUDGET_BYTES == 16 * 2 ** 30
    assert cr.LIMITS[2] == wm.max_features(2) == 3709 and cr.LIMITS[10] == wm.max_features(10) == 950
    two, two20, ten = cr.budget_bytes(10, 3709, 2, 10), cr.budget_bytes(20, 3709, 2, 20), cr.budget_bytes(10, 950, 10, 10)
    assert max(two, two20, ten) <= cr.BUDGET_BYTES                                   # a 10-fold CV at both limits fits
    assert round(two / 1e9, 2) == 2.87 and round(two20 / 1e9, 2) == 5.63 and round(ten / 1e9, 2) == 0.19
    assert cr.budget_bytes(847, 1000, 2, 847) <= cr.BUDGET_BYTES < cr.budget_bytes(848, 1000, 2, 848) and cr.groups_over_budget(1000, 2) == 848
    # from 1024 tile pairs on a group is one chunk whatever n is; below, the chunks are cut at the groups' ends
    assert cr.tile_pairs(3709 + 3) == 27028 and cr.row_chunks(10 ** 6, 3709, 2, [10 ** 5] * 10) == 10
    assert cr.rows_per_chunk(600, 199) == 256 and cr.row_chunks(600, 196, 2, [200, 200, 200]) == 3
    assert cr.row_chunks(600, 196, 2, [257, 343]) == 4
    # sparse x has no partial tiles
    assert cr.budget_bytes(10, 3709, 2, 0) == two - 8 * 10 * 27028 * 256
    # Pa^2 of every accepted shape fits cov_total_kernel's int
    assert (4531 + 2) ** 2 < 2 ** 31


def test_native_refusals_name_the_condition():
    import scipy.sparse as sp

    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    rng = np.random.default_rng(0)
    limit = sa.wmcovariance_max_features(2)
    assert limit == cr.LIMITS[2]

    def refused(code, needle, x, y, foldid, fits=None):
        with pytest.raises(sa.SgdnetError) as e:
            (fits or sa.cv_wmcovariance_fits)(x, y, foldid, 0.5, np.array([0.1, 0.01]))
        assert e.value.code == code and needle in str(e.value), str(e.value)
        return str(e.value)

    wide = rng.standard_normal((6, limit + 1))
    refused(-5, "mode = wmcovariance needs no more features than sgdnet_wmcovariance_max_features(n_classes)", wide, wide[:, :2],
            np.arange(6) % 3)
    refused(-5, "mode = wmcovariance needs no more features", sp.csc_matrix(wide), wide[:, :2], np.arange(6) % 3)
    # the byte budget, from the constant: the fewest one-row groups that are over it at 1000 features (x itself is 6.8 MB)
    p = 1000
    G = cr.groups_over_budget(p, 2)
    big = rng.standard_normal((G, p))
    msg = refused(-5, "mode = wmcovariance needs the moments and the scaled matrices of the groups within %d bytes" % cr.BUDGET_BYTES, big,
                  big[:, :2], np.arange(G))
    assert int(re.search(r"are (\d+) bytes", msg).group(1)) == cr.budget_bytes(G, p, 2, G) > cr.BUDGET_BYTES      # the message gives the bytes
    assert cr.budget_bytes(G - 1, p, 2, G - 1) <= cr.BUDGET_BYTES
    # more than 65 535 groups: sparse x (the groups themselves) and dense x (at least a row chunk per group)
    many = rng.standard_normal((70000, 1))
    y_many = np.column_stack([many[:, 0], -many[:, 0]])
    refused(-5, "mode = wmcovariance needs at most 65535 groups of sparse rows", sp.csc_matrix(many), y_many, np.arange(70000))
    refused(-5, "mode = wmcovariance needs at most 65535 row chunks of the groups", many, y_many, np.arange(70000))
    # the narrow CV refuses what it always refused, by its own name
    x196 = rng.standard_normal((30, 196))
    refused(-5, "mode = mcovariance needs no more features than sgdnet_mcovariance_max_features(n_classes)", x196, x196[:, :2],
            np.arange(30) % 3, fits=sa.cv_mcovariance_fits)

    # what cv_wmcovariance_fits cannot express goes through the C ABI directly
    L = sa.load()
    K = 3
    x = rng.standard_normal((60, 4))
    y = x[:, :K] + rng.standard_normal((60, K))
    xf, yf, f32 = np.asfortranarray(x), np.asfortranarray(y), np.ascontiguousarray(np.arange(60) % 3, dtype=np.int32)

    def call(fold_arr=f32, n_groups=3, lam_arr=np.array([[0.1, 0.01]]), alphas=np.array([0.5]), train_on_rest=0, sparse=False, **ctl_fields):
        ctl = _lib.Control()
        ctl.family, ctl.intercept, ctl.standardize, ctl.max_iter, ctl.tol, ctl.n_lambda, ctl.n_classes = 3, 1, 1, 100, 1e-7, 2, K
        ctl.mode = _lib.MODE_WMCOVARIANCE
        for k, v in ctl_fields.items():
            setattr(ctl, k, v)
        out = [np.zeros(3 * 2 * K), np.zeros(3 * 2 * K * 4), np.zeros(3 * 2), np.zeros(3 * 2), np.zeros(3), np.zeros(3)]
        res = _lib.CvMcovResult(*[_lib.dptr(a) for a in out])
        tail = (_lib.dptr(yf), fold_arr.ctypes.data_as(C.POINTER(C.c_int32)), n_groups, train_on_rest, C.byref(ctl), 1, _lib.dptr(alphas),
                _lib.dptr(lam_arr), C.byref(res))
        if sparse:
            xs = sp.csc_matrix(x)
            colptr, rowidx = np.ascontiguousarray(xs.indptr, dtype=np.int32), np.ascontiguousarray(xs.indices, dtype=np.int32)
            vals = np.ascontiguousarray(xs.data, dtype=np.float64)
            csc = _lib.Csc()
            csc.n_rows, csc.n_cols = 60, 4
            csc.colptr, csc.rowidx = colptr.ctypes.data_as(C.POINTER(C.c_int32)), rowidx.ctypes.data_as(C.POINTER(C.c_int32))
            csc.values = _lib.dptr(vals)
            rc = L.sgdnet_cv_wmcovariance_sparse(C.byref(csc), *tail)
        else:
            rc = L.sgdnet_cv_wmcovariance_dense(_lib.dptr(xf), 60, 4, *tail)
        return rc, L.sgdnet_last_error().decode()

    for sparse in (False, True):
        rc, msg = call(n_gpus=2, sparse=sparse)
        assert rc == -5 and msg.startswith("mode = wmcovariance needs one GPU"), msg
        rc, msg = call(debug=1, sparse=sparse)
        assert rc == -5 and msg.startswith("mode = wmcovariance needs debug = 0"), msg
        for family in (0, 1, 2):
            rc, msg = call(family=family, sparse=sparse)
            assert rc == -5 and msg.startswith("mode = wmcovariance needs family = mgaussian"), msg
        for n_classes in (1, 0):
            rc, msg = call(n_classes=n_classes, sparse=sparse)
            assert rc == -5 and msg.startswith("mode = wmcovariance needs at least two responses"), msg
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
    assert rc == -1 and "sgdnet_cv_wmcovariance" in msg and "train_on_rest needs two groups" in msg, msg


def test_python_argument_checks():
    import sgdnet_amd as sa
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = x[:, :3] + rng.standard_normal((60, 3))
    fold = np.arange(60) % 3
    for needle, kw in (("'separate' or 'batched'", dict(fold_fits="fused")), ("'fold' or 'rest'", dict(train_on="others")),
                       ("'fold' or 'rest'", dict(train_on="others", fold_fits="batched"))):
        with pytest.raises(ValueError) as e:
            sa.cv_sgdnet_wmcovariance(x, y, nfolds=3, **kw)
        assert needle in str(e.value), str(e.value)
    with pytest.raises(TypeError):
        sa.cv_sgdnet_wmcovariance(x, y, nfolds=3, mode="mcovariance")                     # the mode is not an argument
    with pytest.raises(ValueError, match="one array per alpha"):
        sa.cv_wmcovariance_fits(x, y, fold, [0.5, 1.0], [[0.1, 0.01]])
    with pytest.raises(ValueError, match="must be positive"):
        sa.cv_wmcovariance_fits(x, y, fold, 0.5, [0.1, -0.01])
    with pytest.raises(ValueError, match="'fold' or 'rest'"):
        sa.cv_wmcovariance_fits(x, y, fold, 0.5, [0.1], train_on="others")
    with pytest.raises(ValueError, match="must not be one-dimensional"):
        sa.cv_wmcovariance_fits(x, y[:, 0], fold, 0.5, [0.1])                             # K = 1 never reaches the library
    with pytest.raises(ValueError):
        sa.cv_wmcovariance_fits(x, y[:-1], fold, 0.5, [0.1])

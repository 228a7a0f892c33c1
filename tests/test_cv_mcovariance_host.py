"""Cross-validation in multi-response covariance mode (sgdnet_cv_mcovariance_*, sgdnet_amd/csrc/covariance.hip), the parts a
CPU can check.

pooled_problem() restates in numpy what the device does for K responses: per-fold moments of the augmented rows
[x - a | y_1 - a_y1 .. y_K - a_yK | 1] about ONE centre (the whole-data means; 0 for the features where they are not
centred), pooled into a training set T (one fold, or the total -- summed in fold order -- minus one) and re-centred to T's
own means t, d = t - a:

    M^T_jk = C^T_jk - d_j s^T_k - d_k s^T_j + n_T d_j d_k

over all p + K columns, response column r divided by sd_T(y_r) with standardize_response, and from it the scaled Gram
matrix S (p x p) and c~ (p x K) the path kernel iterates on.  direct_problem() forms the same from x[T], y[T] alone, as
fit_mcovariance (driver_direct.cpp) prepares it.  The two must agree to rounding: POOLING_BOUND = 1e-12 is asserted, the bound
of tests/test_cv_covariance_host.py.  The largest difference over the cases below is printed; it was 1.21e-14 when the
test was written, so the pooling itself stays almost five orders of magnitude inside the 1e-9 the GPU tests hold the coefficients to.

The refusals of the native entry points that are decided before a device is looked for, and those of cv_mcovariance_fits
and cv_sgdnet_mcovariance, are checked here too: they need no GPU."""
import numpy as np
import pytest

# (n, p, K, folds): the shapes of tests/test_gpu_cv_mcovariance.py (195, 174 and 63 are sgdnet_mcovariance_max_features(2 / 10 / 96))
SHAPES = [(37, 2, 3, 3), (120, 16, 4, 3), (195, 13, 5, 3), (192, 14, 2, 3), (1003, 33, 3, 10), (1200, 195, 2, 3), (1200, 174, 10, 3),
          (600, 63, 96, 3)]
POOLING_BOUND = 1e-12


def problem(n, p, K, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * n + 31 * p + K)
    x = rng.standard_normal((n, p)) * rng.uniform(0.5, 3.0, p) + rng.uniform(-2.0, 2.0, p)
    B = rng.standard_normal((p, K)) * (rng.random(p) < 0.5)[:, None]
    return x, x @ B + 0.5 * rng.standard_normal((n, K)) * rng.uniform(0.5, 2.0, K) + rng.uniform(-2.0, 2.0, K)


def random_folds(n, G, seed=0):
    return np.random.default_rng(seed).permutation(np.arange(n) % G)


def sorted_folds(x, G):
    """folds cut along a sorted column: every fold's mean of that column sits far from the global mean"""
    fold = np.empty(x.shape[0], dtype=np.int64)
    fold[np.argsort(x[:, 0], kind="stable")] = np.arange(x.shape[0]) * G // x.shape[0]
    return fold


def finish(M, nT, p, standardize, standardize_response):
    """from the (p + K) x (p + K) cross-products about T's own means: S, c~ (p x K) and y~'y~"""
    var = np.diag(M) / nT
    sd_all = np.where(var > 0, np.sqrt(np.where(var > 0, var, 1.0)), 1.0)
    sd = sd_all[:p] if standardize else np.ones(p)
    sd_y = sd_all[p:] if standardize_response else np.ones(M.shape[0] - p)
    return M[:p, :p] / nT / np.outer(sd, sd), M[:p, p:] / sd_y / nT / sd[:, None], (np.diag(M)[p:] / sd_y / sd_y).sum()


def pooled_problem(x, y, fold, G, t, rest, standardize=True, centre=True, standardize_response=False):
    n, p = x.shape
    nc = p + y.shape[1]
    a = np.concatenate([x.mean(axis=0) if centre else np.zeros(p), y.mean(axis=0)])
    aug = np.column_stack([np.column_stack([x, y]) - a, np.ones(n)])
    Cg = np.array([aug[fold == g].T @ aug[fold == g] for g in range(G)])
    C = Cg[t]
    if rest:
        total = np.zeros_like(C)
        for g in range(G):
            total = total + Cg[g]
        C = total - Cg[t]
    nT, s = C[nc, nc], C[:nc, nc]
    d = s / nT
    if not centre:
        d[:p] = 0.0
    M = C[:nc, :nc] - np.outer(d, s) - np.outer(s, d) + nT * np.outer(d, d)
    return finish(M, nT, p, standardize, standardize_response)


def direct_problem(x, y, standardize=True, centre=True, standardize_response=False):
    n, p = x.shape
    z = np.column_stack([x - (x.mean(axis=0) if centre else 0.0), y - y.mean(axis=0)])
    return finish(z.T @ z, float(n), p, standardize, standardize_response)


def difference(got, ref):
    (S, c, yy), (S0, c0, yy0) = got, ref
    return max(np.abs(S - S0).max() / np.abs(S0).max(), np.abs(c - c0).max() / max(np.abs(c0).max(), 1e-300), abs(yy - yy0) / yy0)


def test_pooled_moments_are_the_direct_ones():
    worst = 0.0
    for n, p, K, G in SHAPES:
        x, y = problem(n, p, K)
        for fold in (random_folds(n, G), sorted_folds(x, G)):
            for rest in (False, True):
                for standardize, centre, std_y in ((True, True, False), (False, True, False), (False, False, False), (True, True, True)):
                    for t in range(G):
                        T = (fold != t) if rest else (fold == t)
                        err = difference(pooled_problem(x, y, fold, G, t, rest, standardize, centre, std_y),
                                         direct_problem(x[T], y[T], standardize, centre, std_y))
                        worst = max(worst, err)
                        assert err <= POOLING_BOUND, (n, p, K, G, rest, standardize, centre, std_y, t, err)
    print("pooled vs direct S / c~ / y~'y~: largest relative difference %.3g" % worst)


def test_pooling_with_a_large_mean_column_does_not_cancel():
    """a column of mean 1e6 and sd 1: deviations are taken from the whole-data mean BEFORE anything is multiplied, so the
    correction s s' / n_T is of the order of the column's variance, not of its squared mean.  What is left is the rounding of
    the stored entries themselves (1e6 * 2^-53 = 1.2e-10 absolute on deviations of order 1), which x[T] suffers as well."""
    n, p, K, G = 195, 13, 5, 3
    x, y = problem(n, p, K, seed=1)
    x[:, 3] = 1e6 + np.random.default_rng(5).standard_normal(n)
    for fold in (random_folds(n, G), sorted_folds(x[:, [3]], G)):
        for rest in (False, True):
            for t in range(G):
                T = (fold != t) if rest else (fold == t)
                S, c, _ = pooled_problem(x, y, fold, G, t, rest)
                S0, c0, _ = direct_problem(x[T], y[T])
                assert np.abs(S - S0).max() <= 1e-8 and np.abs(c - c0).max() <= 1e-8


# ---- refusals that need no device ----

def native_refusal(code, needle, x, y, foldid, alpha=0.5, lam=(0.1, 0.01), **kw):
    import sgdnet_amd as sa
    with pytest.raises(sa.SgdnetError) as e:
        sa.cv_mcovariance_fits(x, y, foldid, alpha, np.asarray(lam, dtype=float), **kw)
    assert e.value.code == code and needle in str(e.value), str(e.value)


def test_native_refusals_name_the_condition():
    import ctypes as C

    import scipy.sparse as sp

    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    rng = np.random.default_rng(0)
    K = 3
    x = rng.standard_normal((60, 4))
    y = x[:, :K] + rng.standard_normal((60, K))
    fold = np.arange(60) % 3
    wide = rng.standard_normal((30, sa.mcovariance_max_features(K) + 1))
    native_refusal(-5, "mode = mcovariance needs no more features than sgdnet_mcovariance_max_features(n_classes)", wide, wide[:, :K],
                   np.arange(30) % 3)
    native_refusal(-5, "mode = mcovariance needs no more features", sp.csc_matrix(wide), wide[:, :K], np.arange(30) % 3)
    # leave-one-out at 193 features and 3 responses: 300 groups x 197^2 doubles are 93 MB
    big = rng.standard_normal((300, sa.mcovariance_max_features(K)))
    native_refusal(-5, "mode = mcovariance needs the group moments within", big, big[:, :K], np.arange(300))
    # more than 65 535 groups: sparse x (the groups themselves) and dense x (at least a row chunk per group)
    many = rng.standard_normal((70000, 1))
    y_many = np.column_stack([many[:, 0], -many[:, 0]])
    native_refusal(-5, "mode = mcovariance needs at most 65535 groups of sparse rows", sp.csc_matrix(many), y_many, np.arange(70000))
    native_refusal(-5, "mode = mcovariance needs at most 65535 row chunks of the groups", many, y_many, np.arange(70000))

    # what cv_mcovariance_fits cannot express goes through the C ABI directly
    L = sa.load()
    xf, yf, f32 = np.asfortranarray(x), np.asfortranarray(y), np.ascontiguousarray(fold, dtype=np.int32)
    alphas, lam = np.array([0.5]), np.array([[0.1, 0.01]])

    def call(fold_arr=f32, n_groups=3, lam_arr=lam, mixes=alphas, **ctl_fields):
        ctl = _lib.Control()
        ctl.family, ctl.intercept, ctl.standardize, ctl.max_iter, ctl.tol, ctl.n_lambda, ctl.n_classes = 3, 1, 1, 100, 1e-7, 2, K
        for k, v in ctl_fields.items():
            setattr(ctl, k, v)
        out = [np.zeros(3 * 2 * K), np.zeros(3 * 2 * K * 4), np.zeros(3 * 2), np.zeros(3 * 2), np.zeros(3), np.zeros(3)]
        res = _lib.CvMcovResult(*[_lib.dptr(a) for a in out])
        rc = L.sgdnet_cv_mcovariance_dense(_lib.dptr(xf), 60, 4, _lib.dptr(yf), fold_arr.ctypes.data_as(C.POINTER(C.c_int32)), n_groups, 0,
                                           C.byref(ctl), 1, _lib.dptr(mixes), _lib.dptr(lam_arr), C.byref(res))
        return rc, L.sgdnet_last_error().decode()

    rc, msg = call(n_gpus=2)
    assert rc == -5 and msg.startswith("mode = mcovariance needs one GPU"), msg
    rc, msg = call(debug=1)
    assert rc == -5 and msg.startswith("mode = mcovariance needs debug = 0"), msg
    for family in (0, 1, 2):
        rc, msg = call(family=family)
        assert rc == -5 and msg.startswith("mode = mcovariance needs family = mgaussian"), msg
    for n_classes in (1, 0):
        rc, msg = call(n_classes=n_classes)
        assert rc == -5 and msg.startswith("mode = mcovariance needs at least two responses"), msg
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
    assert rc == -1 and "lambdas[0][1]" in msg and "negative" in msg, msg
    rc, msg = call(mixes=np.array([1.5]))
    assert rc == -1 and "alphas[0] = 1.5" in msg, msg


def test_python_refusals_name_the_condition():
    import sgdnet_amd as sa
    assert "cv_mcovariance_fits" in sa.__all__ and "cv_sgdnet_mcovariance" in sa.__all__
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = x[:, :3] + rng.standard_normal((60, 3))
    fold = np.arange(60) % 3
    with pytest.raises(ValueError, match="one array per alpha"):
        sa.cv_mcovariance_fits(x, y, fold, [0.5, 1.0], [[0.1, 0.01]])
    with pytest.raises(ValueError, match="must be positive"):
        sa.cv_mcovariance_fits(x, y, fold, 0.5, [0.1, -0.01])
    with pytest.raises(ValueError, match="'fold' or 'rest'"):
        sa.cv_mcovariance_fits(x, y, fold, 0.5, [0.1], train_on="others")
    with pytest.raises(ValueError, match="must not be one-dimensional"):
        sa.cv_mcovariance_fits(x, y[:, 0], fold, 0.5, [0.1])
    with pytest.raises(ValueError, match="'separate' or 'batched'"):
        sa.cv_sgdnet_mcovariance(x, y, nfolds=3, fold_fits="fused")
    with pytest.raises(ValueError, match="'fold' or 'rest'"):
        sa.cv_sgdnet_mcovariance(x, y, nfolds=3, fold_fits="batched", train_on="others")
